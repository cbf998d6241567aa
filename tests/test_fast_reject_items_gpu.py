"""k_fast_cells's rejection test enumerates the detection dwords dw_lo..dw_hi of a band's rows, run R of 64 items on wave R % 4
(fc_item_* in csrc/orb_device.h; tests/test_fast_reject_items_cpu.py holds the enumeration itself).  Here the kernel, on frame
sizes whose bands have the shapes that matter -- one-cell bands of 7 detection dwords in a row of 12, four-cell pitch-144 bands
of 16 runs dealt 4 / 4 / 4 / 4, a pitch-128 band of 20 runs, three-cell bands starting at dword 1 and at dword 2, a two-cell band
of 7 runs dealt 2 / 2 / 2 / 1 -- and on three kinds of image: cropped synthetic frames, images dense in survivors of the
rejection test (all four pixel slots of most runs push, a wave's stack passes 63 between runs), and images whose only corners
sit in the first and last detection column and row of every cell.  Every case extracts a 2-frame batch and compares, per frame
and level, the FAST candidates, and the keypoints and descriptors, with the CPU oracle.  The stated property of each input and
of each frame size's band plan is asserted first."""
import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.orb import ORBextractor

import fc_band_plan_ref as plan

pytestmark = pytest.mark.gpu

NF, SF, INI, MN = 300, 1.2, 20, 7
BORDER = 16                                   # candidate coordinates are relative to the detection area's corner (19 - 3)
SHAPES = [(182, 96, 2), (230, 80, 1), (100, 64, 1)]
_key = lambda b: (b["pitch"], b["bh"], b["dw_lo"], b["dw_hi"])


def _check(ctx, oracle, frames, nlevels):
    """frames [2, h, w] on the device, rows (w rounded up to 4) apart; candidates of every level, keypoints and descriptors
    against the oracle."""
    import torch
    n, h, w = frames.shape
    stride = (w + 3) & ~3
    plane = stride * h + 64
    host = np.random.default_rng(w * 1000 + h).integers(0, 256, plane * n + 4096, dtype=np.uint8)
    for f in range(n):
        np.lib.stride_tricks.as_strided(host[f * plane:], shape=(h, w), strides=(stride, 1))[...] = frames[f]
    buf = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    ex = ORBextractor(NF, SF, nlevels, INI, MN, ctx=ctx)
    ex.extract_dev(buf.data_ptr(), w, h, stride, plane, n)
    kps, desc, counts = ex.fetch()
    par = oracle.default_params(NF, SF, nlevels, INI, MN)
    for f in range(n):
        for l in range(nlevels):
            r = oracle.orb_extract(par, frames[f], cand_level=l)
            xy, sc = ex.fast_candidates(f, l)
            assert len(xy) == len(r["cand_xy"]) and (xy == r["cand_xy"]).all() and (sc == r["cand_score"]).all(), (f, l)
        c = int(counts[f])
        assert c == len(r["kps"]), f
        for name in kps.dtype.names:
            assert (kps[f, :c][name] == r["kps"][name]).all(), (f, name)
        assert (desc[f, :c] == r["desc"]).all(), f
    del buf


def _assert_plan(shape):
    """What the frame size is here for."""
    w, h, nl = shape
    bands = plan.bands(w, h, nl)
    geo = [(b["level"], b["ncells"]) + _key(b) for b in bands]
    if shape == (182, 96, 2):
        assert (0, 1, 48, 38, 1, 7) in geo                                   # one cell: 7 detection dwords of 12
        assert (0, 4, 144, 38, 1, 31) in geo and plan.wave_runs((144, 38, 1, 31)) == [4, 4, 4, 4]      # the bench's dominant band
        assert [g for g in geo if g[0] == 1] == [(1, 4, 128, 48, 1, 30)] and plan.runs((128, 48, 1, 30)) == 20
    elif shape == (230, 80, 1):
        assert geo == [(0, 3, 128, 48, 1, 26), (0, 3, 112, 48, 2, 25)]
    else:
        assert geo == [(0, 2, 80, 32, 1, 17)] and plan.wave_runs((80, 32, 1, 17)) == [2, 2, 2, 1]
    return bands


def _survivors(img, t):
    """Per pixel: passes the rejection test at threshold t (the compass pixels allow the brighter or the darker polarity)."""
    a = img.astype(np.int32)
    h, w = a.shape
    v = a[3:h - 3, 3:w - 3]
    n, s, e, wst = a[6:h, 3:w - 3], a[0:h - 6, 3:w - 3], a[3:h - 3, 6:w], a[3:h - 3, 0:w - 6]
    out = np.zeros((h, w), bool)
    out[3:h - 3, 3:w - 3] = (np.minimum(np.maximum(n, s), np.maximum(e, wst)) > v + t) | \
                            (np.maximum(np.minimum(n, s), np.minimum(e, wst)) < v - t)
    return out


def _run_figures(img, band):
    """Level-0 band: (runs, runs with a survivor in each of the four pixel slots, a wave's stack passes 63 with a run to follow),
    from the enumeration the kernel runs (ccm_debug_fc_items) and the survivors of the rejection test on the image."""
    g = _key(band)
    out = np.zeros((65 * 64, 6), np.int32)
    n = _lib.load().ccm_debug_fc_items(*g, _lib.ptr(out), len(out))
    run, wave, lane, row, dw, pos0 = out[:n].T
    surv = _survivors(img, min(INI, MN))
    nruns = plan.runs(g)
    slot = np.zeros((nruns, 4), int)
    for i in range(4):
        col = 4 * dw + i
        s = surv[band["y0"] + row, np.minimum(band["xa"] + col, img.shape[1] - 1)] & (col >= band["c_lo"]) & (col < band["c_hi"])
        slot[:, i] = np.bincount(run, weights=s, minlength=nruns)
    stack, passes = [0, 0, 0, 0], False
    for r in range(nruns):
        stack[r % 4] += int(slot[r].sum())
        if r + 4 < nruns:
            passes |= stack[r % 4] > 63
            stack[r % 4] %= 64
    return nruns, int((slot > 0).all(axis=1).sum()), passes


def _crop(frames, w, h):
    return np.ascontiguousarray(frames[:, 120:120 + h, 300:300 + w])


@pytest.fixture(scope="module")
def synth_frames():
    return synth.frames(0, 2)


@pytest.mark.parametrize("shape", SHAPES)
def test_synth_cropped(ctx, oracle, synth_frames, shape):
    w, h, nl = shape
    _assert_plan(shape)
    frames = _crop(synth_frames, w, h)
    par = oracle.default_params(NF, SF, nl, INI, MN)
    assert all(len(oracle.orb_extract(par, f, cand_level=0)["cand_xy"]) > 0 for f in frames)
    _check(ctx, oracle, frames, nl)


def _dense(w, h):
    y, x = np.indices((h, w))
    noise = np.random.default_rng(w + h).integers(0, 256, (h, w), dtype=np.uint8)
    ramp = np.clip((3 * (x + y)) % 200 + 20 + np.random.default_rng(9).integers(-40, 41, (h, w)), 0, 255).astype(np.uint8)
    return np.stack([noise, ramp])


@pytest.mark.parametrize("shape", SHAPES)
def test_dense_survivors(ctx, oracle, shape):
    """More than a quarter of the detection area survives the rejection test; in every level-0 band most runs push in all four
    pixel slots, and in every band of more than four runs a wave's stack passes 63 with a run to follow."""
    w, h, nl = shape
    bands = _assert_plan(shape)
    frames = _dense(w, h)
    for img in frames:
        assert _survivors(img, min(INI, MN))[19:h - 19, 19:w - 19].mean() > 0.25
        for b in bands:
            if b["level"] == 0:
                nruns, four, passes = _run_figures(img, b)
                assert 2 * four > nruns, (b, nruns, four)
                assert passes or nruns <= 4, b
    _check(ctx, oracle, frames, nl)


def _edge_corners(w, h, bands, up):
    """A flat image with one pixel 30 above (below) it in the first and in the last detection column, and in the first and in the
    last detection row, of every level-0 cell; the four are kept more than 3 apart from those of the neighbouring cells."""
    img = np.full((h, w), 100, np.uint8)
    want = []
    for b in bands:
        if b["level"]:
            continue
        for x0, y0, cw, ch in b["cells"]:
            xf, xl, yf, yl = x0 + 3, x0 + cw - 4, y0 + 3, y0 + ch - 4
            xm, ym = (xf + xl) // 2, (yf + yl) // 2
            want += [(xf, ym - 5), (xl, ym + 5), (xm - 5, yf), (xm + 5, yl)]
    for x, y in want:
        img[y, x] = 130 if up else 70
    return img, want


@pytest.mark.parametrize("shape", SHAPES)
def test_corners_on_the_range_ends(ctx, oracle, shape):
    w, h, nl = shape
    bands = _assert_plan(shape)
    imgs, wants = zip(*[_edge_corners(w, h, bands, up) for up in (True, False)])
    par = oracle.default_params(NF, SF, nl, INI, MN)
    for img, want in zip(imgs, wants):
        r = oracle.orb_extract(par, img, cand_level=0)
        got = {(int(x) + BORDER, int(y) + BORDER) for x, y in r["cand_xy"]}
        assert got == set(want) and len(r["cand_xy"]) == len(want) == 4 * sum(b["ncells"] for b in bands if b["level"] == 0)
    _check(ctx, oracle, np.stack(imgs), nl)
