"""k_orient_desc's orientation and steering through ccm_debug_od_steer -- one wave per moment pair, running the device functions the
kernel runs for fastAtan2, for (cos, sin) and for the steered, rounded sample points -- against a numpy transcription: fastAtan2
in float32 operations, include/ccm_sincos.h in float64 operations with its one cast to float32, the steering in float32 multiply
and add, np.rint for the rounding.  numpy's elementwise IEEE arithmetic does not contract, so every comparison is for equality.
Then the whole kernel against the CPU oracle, row for row, on edge frames at the two smallest batches that select each of its forms."""
import os
import re

import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.orb import ORBextractor, lane_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 752, 480
M_MAX = 15 * 255 * 709             # the largest moment: 709 pixels in the radius-15 disc, u <= 15, pixels <= 255


def _pattern():
    with open(os.path.join(ROOT, "include", "ccm_orb_pattern.h")) as fh:
        body = fh.read().split("{", 1)[1].split("}", 1)[0]
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], np.float32).reshape(512, 2)


# ------------------------------------------------------------------------------------------------- the transcription
def _atan2_deg(y, x):
    """cv::fastAtan2 in float32 operations: both arms as written there, selected by ax >= ay."""
    f = np.float32
    scale = f(180.0 / np.pi)
    p1, p3, p5, p7 = f(0.9997878412794807) * scale, f(-0.3258083974640975) * scale, f(0.1555786518463281) * scale, f(-0.04432655554792128) * scale
    eps = f(2.2204460492503131e-16)
    ax, ay = np.abs(x), np.abs(y)

    def poly(c):
        c2 = c * c
        return (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    with np.errstate(over="ignore", invalid="ignore"):               # (the arm that is not taken may overflow)
        a = np.where(ax >= ay, poly(ay / (ax + eps)), f(90) - poly(ax / (ay + eps)))
    a = np.where(x < 0, f(180) - a, a)
    a = np.where(y < 0, f(360) - a, a)
    assert a.dtype == np.float32
    return a


def _sincos(xf):
    """include/ccm_sincos.h in float64 operations: (sin, cos) as float32, and k."""
    x = xf.astype(np.float64)
    k = (x * 0.63661977236758134308 + 0.5).astype(np.int64)
    kd = k.astype(np.float64)
    r = x - kd * 1.57079632673412561417e+00
    r = r - kd * 6.07710050650619224932e-11
    z = r * r
    ps = np.full_like(z, -1.0 / 355687428096000.0)
    for c in (1.0 / 1307674368000.0, -1.0 / 6227020800.0, 1.0 / 39916800.0, -1.0 / 362880.0, 1.0 / 5040.0, -1.0 / 120.0, 1.0 / 6.0):
        ps = ps * z + c
    sr = r - (r * z) * ps
    pc = np.full_like(z, 1.0 / 6402373705728000.0)
    for c in (-1.0 / 20922789888000.0, 1.0 / 87178291200.0, -1.0 / 479001600.0, 1.0 / 3628800.0, -1.0 / 40320.0, 1.0 / 720.0, -1.0 / 24.0, 0.5):
        pc = pc * z + c
    cr = 1.0 - z * pc
    q = k & 3
    s = np.choose(q, [sr, cr, -sr, -cr])
    c = np.choose(q, [cr, -sr, -cr, sr])
    return s.astype(np.float32), c.astype(np.float32), k


def _angle_ab(m01, m10):
    angle = _atan2_deg(m01.astype(np.float32), m10.astype(np.float32))
    b, a, k = _sincos(angle * np.float32(np.pi / 180.0))            # (:103-105: a = cos, b = sin)
    return angle, a, b, k


def _expected(m01, m10):
    angle, a, b, k = _angle_ab(m01, m10)
    p = _pattern()
    px, py = p[None, :, 0], p[None, :, 1]
    dx = np.rint(px * a[:, None] - py * b[:, None])                  # (:107-110, cvRound)
    dy = np.rint(px * b[:, None] + py * a[:, None])
    assert dx.dtype == np.float32
    return angle, a, b, np.stack([dx, dy], -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------- the inputs
def _near_multiples_of_45():
    """For each multiple of 45 degrees, the small integer moment pairs whose angle lies nearest below it and nearest at or above it:
    at the odd multiples k = (int)(x 2/pi + 0.5) switches quadrant, at the even ones the reduced argument changes sign (and at 360
    k reaches 4).  Returns the pairs and, per multiple, the set of k on either side."""
    n = 48
    j, i = np.meshgrid(np.arange(-n, n + 1, dtype=np.int32), np.arange(-n, n + 1, dtype=np.int32))
    m01, m10 = i.ravel(), j.ravel()
    angle, _, _, k = _angle_ab(m01, m10)
    pairs, sides = [], {}
    for m in range(9):
        d = angle.astype(np.float64) - 45.0 * m
        for below in (True, False):
            idx = np.nonzero(d < 0 if below else d >= 0)[0]
            idx = idx[np.argsort(np.abs(d[idx]), kind="stable")[:64]]
            pairs.append(np.stack([m01[idx], m10[idx]], 1))
            sides[(m, below)] = set(k[idx].tolist())
    return np.concatenate(pairs), sides


def _inputs():
    signs = [(s, t) for s in (-1, 1) for t in (-1, 1)]
    mags = [1, 2, 3, 7, 255, 256, 4095, 65535, 65536, 1 << 20, (1 << 21) + 1, M_MAX - 1, M_MAX]
    rows = [(0, 0)]
    for v in mags:
        rows += [(0, v), (0, -v), (v, 0), (-v, 0)]                   # one moment zero, every sign of the other
        rows += [(s * v, t * v) for s, t in signs]                   # |m01| == |m10|: the ax >= ay tie
    for s, t in signs:
        rows += [(s * M_MAX, t), (s, t * M_MAX)]                     # the extreme moments against +-1
    near, sides = _near_multiples_of_45()
    rng = np.random.default_rng(20240)
    rnd = rng.integers(-M_MAX, M_MAX + 1, (4096, 2))
    allp = np.concatenate([np.array(rows), near, rnd]).astype(np.int32)
    return np.ascontiguousarray(allp[:, 0]), np.ascontiguousarray(allp[:, 1]), sides


def test_quadrant_switches_are_covered():
    """(host only) the inputs reach all four values of k & 3 and both sides of each quadrant switch of ccm_sincosf."""
    m01, m10, sides = _inputs()
    assert 5000 <= len(m01) <= 7000
    k = _angle_ab(m01, m10)[3]
    assert set((k & 3).tolist()) == {0, 1, 2, 3}
    for m in (1, 3, 5, 7):                                           # 45, 135, 225, 315 degrees: k goes from (m - 1) / 2 to (m + 1) / 2
        assert (m - 1) // 2 in sides[(m, True)] and (m + 1) // 2 in sides[(m, False)], (m, sides[(m, True)], sides[(m, False)])
    assert 4 in sides[(8, True)] and 0 in sides[(0, False)]          # just below 360 degrees and at 0


def test_angle_sincos_and_steered_points(ctx):
    m01, m10, _ = _inputs()
    n = len(m01)
    angle = np.empty(n, np.float32); ab = np.empty((n, 2), np.float32); offs = np.empty((n, 512, 2), np.int8)
    ctx.check(_lib.load().ccm_debug_od_steer(ctx.handle, _lib.ptr(m01), _lib.ptr(m10), n, _lib.ptr(angle), _lib.ptr(ab), _lib.ptr(offs)))
    e_angle, e_a, e_b, e_offs = _expected(m01, m10)
    bad = np.nonzero(angle.view(np.uint32) != e_angle.view(np.uint32))[0]
    assert len(bad) == 0, ("angle", [(int(m01[i]), int(m10[i]), float(angle[i]), float(e_angle[i])) for i in bad[:5]])
    for name, got, exp in (("a", ab[:, 0], e_a), ("b", ab[:, 1], e_b)):
        bad = np.nonzero(got.view(np.uint32) != exp.view(np.uint32))[0]
        assert len(bad) == 0, (name, [(int(m01[i]), int(m10[i]), float(got[i]), float(exp[i])) for i in bad[:5]])
    assert np.abs(e_offs).max() <= 18 and np.abs(offs.astype(np.int32)).max() <= 18
    bad = np.nonzero((offs.astype(np.int32) != e_offs).any((1, 2)))[0]
    assert len(bad) == 0, ("offsets", [(int(m01[i]), int(m10[i])) for i in bad[:5]])


def test_steer_tap_arguments(ctx):
    lib = _lib.load()
    assert "ccm_debug_od_steer" in _lib.SYMBOLS
    one = np.zeros(1, np.int32)
    assert lib.ccm_debug_od_steer(ctx.handle, None, None, 0, None, None, None) == 0
    assert lib.ccm_debug_od_steer(ctx.handle, _lib.ptr(one), _lib.ptr(one), -1, None, None, None) == -1
    assert lib.ccm_debug_od_steer(ctx.handle, _lib.ptr(one), _lib.ptr(one), 1, None, None, None) == -1
    assert lib.ccm_debug_od_steer(None, _lib.ptr(one), _lib.ptr(one), 0, None, None, None) == -1


# ------------------------------------------------------------------------------------------------- the kernel's two forms
def _edge_frame(seed):
    """Noise in a 96-pixel frame along every edge (27 pixels on level 7), flat inside: keypoints only near the edges, whose
    patches take the BORDER_REFLECT_101 path."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W), dtype=np.uint8)
    img[96:H - 96, 96:W - 96] = 128
    return img


def _out_per_frame(ex):
    """The keypoint slots per frame of the extractor's geometry: per level the features wanted + 4, at least 4 per quadtree root."""
    lw, lh = ex.level_sizes(W, H)
    opf = 0
    for l in range(ex.GetLevels()):
        roots = int(np.round(np.float32(lw[l] - 19 + 3 - 16) / np.float32(lh[l] - 19 + 3 - 16)))
        opf += max(int(ex.mnFeaturesPerLevel[l]) + 4, 4 * roots)
    return opf


def _switch_frames(opf):
    """The smallest batch that runs the eight-slots-per-wave form, from the library's chunk plan: a chunk is never smaller than that
    batch, so with L frames per chunk (L above it) a batch of L + 1 frames is cut in two exactly when L + 1 >= 2 * switch."""
    first = next(L for L in range(2, 1 << 16) if len(lane_plan(L + 1, opf, L)) == 2)
    return (first + 1) // 2


def _same(kps, desc, ref, what):
    assert len(kps) == len(ref["kps"]), what
    for name in kps.dtype.names:
        assert (kps[name] == ref["kps"][name]).all(), (what, name)
    bad = np.nonzero((desc != ref["desc"]).any(1))[0]
    assert len(bad) == 0, (what, "descriptor rows differ", bad[:10])


def _row_parities(kps):
    p = _pattern()
    t = np.deg2rad(kps["angle"].astype(np.float64))
    a, b = np.cos(t).astype(np.float32), np.sin(t).astype(np.float32)
    dy = np.rint(p[None, :, 0] * b[:, None] + p[None, :, 1] * a[:, None]).astype(int)
    return set((dy & 1).ravel().tolist())


def test_edge_frames_one_slot_per_wave(ctx, oracle):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    par = oracle.default_params()
    img = _edge_frame(3)
    kps, desc = ex(img)
    _same(kps, desc, oracle.orb_extract(par, img), "single")
    assert _row_parities(kps) == {0, 1} and set((kps["angle"] // 90).astype(int).tolist()) == {0, 1, 2, 3}


def test_edge_frames_eight_slots_per_wave(ctx, oracle):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    par = oracle.default_params()
    opf = _out_per_frame(ex)
    n = _switch_frames(opf)
    assert n > 1 and len(lane_plan(n, opf, 128)) == 1
    imgs = synth.frames(11, n)
    imgs[0] = _edge_frame(3)
    imgs[n // 2] = _edge_frame(4)
    imgs[n - 1] = _edge_frame(5)
    kps, desc, counts = ex.extract_batch(imgs)
    for f in range(n):
        c = int(counts[f])
        _same(kps[f, :c], desc[f, :c], oracle.orb_extract(par, imgs[f]), ("batch", f))
    for f in (0, n // 2, n - 1):
        c = int(counts[f])
        assert _row_parities(kps[f, :c]) == {0, 1} and set((kps[f, :c]["angle"] // 90).astype(int).tolist()) == {0, 1, 2, 3}
