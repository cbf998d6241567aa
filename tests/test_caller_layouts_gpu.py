"""Caller-chosen memory layouts through the C ABI, against the CPU oracle on packed images.

The ABI lets the caller choose the layout of what it passes in: a device base address, an image row stride, an image plane
stride, descriptor pair strides and per-pair live counts on the device.  The kernels pick their staging path from that layout
(dword loads for a 4-byte aligned base and pitch, bytes otherwise), so every case here is run at addresses and pitches that
select each path, with the bytes outside the images filled three different ways, and checked bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.orb import ORBextractor
from motioncheck_ccm_slam_amd.vocabulary import ORBVocabulary, synthetic_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_CAPACITY = -1, -4

# parameter set -> (nfeatures, scaleFactor, nLevels, iniThFAST, minThFAST), w, h
PSETS = {"default": ((1000, 1.2, 8, 20, 7), 752, 480),
         "init641": ((2000, 1.2, 8, 20, 7), 641, 479),       # the initialisation extractor at an odd size: w % 4 == 1
         "kitti": ((1500, 1.2, 8, 20, 7), 1241, 376)}

# (id, parameter set, frames, base offset, row stride, plane stride (None: stride * h), first frame seed)
CASES = [
    ("off1", "default", 2, 1, 752, None, 0),
    ("off2", "default", 2, 2, 752, None, 2),
    ("off3", "default", 2, 3, 752, None, 4),
    ("off4", "default", 2, 4, 752, None, 6),
    ("stride755", "default", 2, 0, 755, None, 8),
    ("stride756", "default", 2, 0, 756, None, 10),
    ("stride768", "default", 2, 0, 768, None, 12),
    ("stride800", "default", 2, 0, 800, None, 14),
    ("plane_gap_odd", "default", 3, 0, 760, 760 * 480 + 37, 16),
    ("single_plane0", "default", 1, 5, 757, 0, 19),
    ("batch41", "default", 41, 0, 756, 756 * 480 + 5, 20),       # k_orient_desc's looping form; frames alternate between the paths
    ("w641_s641", "init641", 2, 0, 641, None, 0),
    ("w641_s642", "init641", 2, 0, 642, None, 2),
    ("w641_s644", "init641", 2, 0, 644, None, 4),               # pitch == round_up(w, 4): the edge of the dword path
    ("w641_single_off2", "init641", 1, 2, 644, 0, 6),
    ("kitti_s1243_off1", "kitti", 1, 1, 1243, 0, 0),
    ("kitti_s1244", "kitti", 2, 0, 1244, None, 1),
]
CASE = {c[0]: c for c in CASES}
FILLS = ("random", 0x00, 0xFF)


def _frame(pset, seed):
    _, w, h = PSETS[pset]
    if (w, h) == (752, 480):
        return synth.frame(seed)
    return synth.frame(seed, w, h, n_rect=max(60, 600 * w * h // (752 * 480)))


def _frames(pset, seed, n):
    return np.stack([_frame(pset, seed + i) for i in range(n)])


_REF = {}


def _ref(oracle, pset, seed, full=False):
    """Oracle results of one frame (cached: cases share frames); full adds the pyramid and the level-0/1 FAST candidates."""
    if (pset, seed, True) in _REF:
        return _REF[(pset, seed, True)]
    if (pset, seed, full) not in _REF:
        par = oracle.default_params(*PSETS[pset][0])
        img = _frame(pset, seed)
        if full:
            r = oracle.orb_extract(par, img, want_levels=True, cand_level=0)
            r1 = oracle.orb_extract(par, img, cand_level=1)
            r["cand1_xy"], r["cand1_score"] = r1["cand_xy"], r1["cand_score"]
        else:
            r = oracle.orb_extract(par, img)
        _REF[(pset, seed, full)] = r
    return _REF[(pset, seed, full)]


def _same(kps, desc, ref, what=""):
    assert len(kps) == len(ref["kps"]), (what, len(kps), len(ref["kps"]))
    for name in kps.dtype.names:
        assert (kps[name] == ref["kps"][name]).all(), (what, name)
    assert (desc == ref["desc"]).all(), what


def _geometry(case):
    _, pset, n, off, stride, plane, _ = case
    _, w, h = PSETS[pset]
    return w, h, n, off, stride, stride * h if plane is None else plane


def _staging_path(base, pitch, w):
    """The level-0 staging path k_fast_cells / k_fast_score take for a frame at `base` (orb_fast_cells.hip, orb_fast_tiles.hip: dword_ok)."""
    return "dword" if ((base | pitch) & 3) == 0 and pitch >= ((w + 3) & ~3) else "byte"


def _case_paths(case):
    """Per frame, for an allocation that is 16-byte aligned (asserted where the frames are placed)."""
    w, h, n, off, stride, plane = _geometry(case)
    return [_staging_path(off + f * plane, stride, w) for f in range(n)]


def _place(frames, stride, plane, offset, fill):
    """A host buffer holding the frames at offset + f * plane with rows `stride` apart; every other byte (row padding, plane
    gaps, the bytes before the offset and a tail after the last frame) is `fill`.  No frame ends at the end of the buffer."""
    n, h, w = frames.shape
    size = offset + plane * (n - 1) + stride * h + 4096
    if fill == "random":
        buf = np.random.default_rng(size).integers(0, 256, size, dtype=np.uint8)
    else:
        buf = np.full(size, fill, np.uint8)
    for f in range(n):
        view = np.lib.stride_tricks.as_strided(buf[offset + f * plane:], shape=(h, w), strides=(stride, 1))
        view[...] = frames[f]
    return buf


def _results(kps, desc, counts):
    """The fetched arrays; the rows past each frame's count are zero, whatever earlier calls on the context left there."""
    for f, c in enumerate(counts):
        assert not kps[f, c:].view(np.uint8).any() and not desc[f, c:].any(), ("stale rows past the count", f)
    return dict(kps=kps, desc=desc, counts=counts)


def _sample(n):
    return sorted({0, 1, n // 2, n - 1} & set(range(n)))


def _extract_dev_case(ex, case, fill, taps=True):
    """Frames of `case` placed in a torch buffer, extracted through ccm_orb_extract_dev; host copies of every result."""
    import torch
    w, h, n, off, stride, plane = _geometry(case)
    buf = torch.from_numpy(_place(_frames(case[1], case[6], n), stride, plane, off, fill)).cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0                   # the staging paths predicted by _case_paths
    ex.extract_dev(buf.data_ptr() + off, w, h, stride, plane, n)
    out = _results(*ex.fetch())
    if taps:
        for f in _sample(n):
            for l in range(ex.GetLevels()):
                out["pyr%d_%d" % (f, l)] = ex.image_pyramid_level(f, l)
            for l in (0, 1):
                xy, sc = ex.fast_candidates(f, l)
                out["cand%d_%d" % (f, l)] = np.concatenate([xy.ravel(), sc])
    del buf
    return out


def _check_vs_oracle(oracle, case, res, what=""):
    _, pset, n, _, _, _, seed = case
    for f in range(n):
        full = f in _sample(n)
        r = _ref(oracle, pset, seed + f, full)
        c = int(res["counts"][f])
        _same(res["kps"][f, :c], res["desc"][f, :c], r, (what, case[0], f))
        if full and "pyr%d_0" % f in res:
            for l in range(len(r["levels"])):
                assert (res["pyr%d_%d" % (f, l)] == r["levels"][l]).all(), (what, case[0], f, "pyramid", l)
            for l, k in ((0, "cand"), (1, "cand1")):
                ref = np.concatenate([r[k + "_xy"].ravel(), r[k + "_score"]])
                got = res["cand%d_%d" % (f, l)]
                assert len(got) == len(ref) and (got == ref).all(), (what, case[0], f, "candidates", l)


def _identical(a, b, what=""):
    assert set(a) == set(b), what
    for k in a:
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), (what, k)


# ------------------------------------------------------------------------------------------------- 1./2. layout matrix, padding
def test_matrix_reaches_both_staging_paths():
    """The layout matrix covers both level-0 staging paths, the exact edge of the dword path, odd source pitches for
    k_pyr_resize's level-1 fetch and k_orient_desc's unaligned patch rows, single frames and the looping descriptor kernel."""
    paths = {p for c in CASES for p in _case_paths(c)}
    assert paths == {"dword", "byte"}
    assert any(_case_paths(c) == ["dword"] * c[2] and c[4] == ((PSETS[c[1]][1] + 3) & ~3) and PSETS[c[1]][1] % 4 for c in CASES)
    assert any(c[4] % 2 and c[4] - PSETS[c[1]][1] < 4 for c in CASES)          # odd pitch with < 4 bytes of row padding
    assert any(c[2] == 1 and c[5] == 0 for c in CASES) and any(c[2] >= 40 for c in CASES)
    ex = ORBextractor(*PSETS["default"][0])
    assert _od_items(ex, 752, 480, 41)[1] == 8 and _od_items(ex, 752, 480, 2)[1] == 1


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_extract_dev_layouts(ctx, oracle, case):
    """Keypoints and descriptors of every frame, pyramid levels 0-7 and the level-0/1 FAST candidates of sampled frames equal
    the oracle's on the packed image; the bytes outside the images (0x00, 0xFF, random) change nothing."""
    ex = ORBextractor(*PSETS[case[1]][0], ctx=ctx)
    runs = {fill: _extract_dev_case(ex, case, fill) for fill in FILLS}
    _check_vs_oracle(oracle, case, runs["random"])
    for fill in FILLS[1:]:
        _identical(runs[fill], runs["random"], (case[0], fill))


# ------------------------------------------------------------------------------------------------- 3./4. switches in child processes
def _od_items(ex, w, h, nframes):
    """(workgroups, slots per wave) of k_orient_desc: its grid is out_per_frame / (4 waves * slots) x frames (orb_orient_desc.hip)."""
    lw, lh = ex.level_sizes(w, h)
    opf = 0
    for l in range(ex.GetLevels()):
        roots = int(np.round(np.float32(lw[l] - 19 + 3 - 16) / np.float32(lh[l] - 19 + 3 - 16)))
        opf += max(int(ex.mnFeaturesPerLevel[l]) + 4, 4 * roots)
    items = 8 if opf * nframes >= 4 * 8192 else 1
    return -(-opf // (4 * items)) * nframes, items


def _fast_bands(ex, w, h):
    """Bands of k_fast_cells (its grid is bands x frames): orb_prepare's FAST cells (ORBextractor.cpp:941-974) cut into runs of
    at most 4 cells of one cell row whose 16-byte aligned tile stays within 144 bytes."""
    lw, lh = ex.level_sizes(w, h)
    nb = 0
    for l in range(ex.GetLevels()):
        maxbx, maxby = int(lw[l]) - 16, int(lh[l]) - 16
        width, height = np.float32(maxbx - 16), np.float32(maxby - 16)
        ncols, nrows = int(width / np.float32(30)), int(height / np.float32(30))
        if ncols < 1 or nrows < 1:
            continue
        wc, hc = int(np.ceil(width / np.float32(ncols))), int(np.ceil(height / np.float32(nrows)))
        for i in range(nrows):
            if 16 + i * hc >= maxby - 3:
                continue
            row = [(x0, min(x0 + wc + 6, maxbx) - x0) for x0 in (16 + j * wc for j in range(ncols)) if x0 < maxbx - 6]
            a = 0
            while a < len(row):
                xa, b = (row[a][0] - 4) & ~3, a
                while b < len(row):
                    pitch = -(-(row[b][0] + row[b][1] + 4 - xa) // 16) * 16
                    if b > a and (pitch > 144 or b - a >= 4):
                        break
                    b += 1
                nb += 1
                a = b
    return nb


XCD_FRAMES = 43
FUSED0_CASES = ("off1", "off3", "stride755", "stride768", "plane_gap_odd", "w641_s641", "w641_s642", "w641_s644", "kitti_s1243_off1")


def _host_gap_view(n, w, h, stride, plane, seed, pset="init641", offset=3):
    frames = _frames(pset, seed, n)
    buf = _place(frames, stride, plane, offset, "random")
    return np.lib.stride_tricks.as_strided(buf[offset:], shape=(n, h, w), strides=(plane, stride, 1)), frames


def _switch_runs():
    """What every switch must leave unchanged, run on a fresh context: a subset of the device layout matrix, a 43-frame batch
    (k_fast_cells and k_orient_desc grids whose item counts are not multiples of 24: the chunk-cyclic order's ragged tail),
    128 packed frames through the host entry point (two upload chunks: the linear mode), and 5 frames of w = 641 at a row stride
    of 656 and a padded plane stride through it (the per-image copy loop, or the linear mode with CCM_ORB_CHUNK=2)."""
    ctx = _lib.Context(0)
    out = {}
    for name in FUSED0_CASES:
        ex = ORBextractor(*PSETS[CASE[name][1]][0], ctx=ctx)
        for k, v in _extract_dev_case(ex, CASE[name], "random").items():
            out["%s:%s" % (name, k)] = v
    ex = ORBextractor(*PSETS["default"][0], ctx=ctx)
    for k, v in _extract_dev_case(ex, ("xcd", "default", XCD_FRAMES, 0, 752, None, 100), "random", taps=False).items():
        out["xcd:" + k] = v
    for k, v in _results(*ex.extract_batch(synth.frames(200, 128))).items():
        out["host128:" + k] = v
    ex = ORBextractor(*PSETS["init641"][0], ctx=ctx)
    view, _ = _host_gap_view(5, 641, 479, 656, 656 * 479 + 48, 30)
    for k, v in _results(*ex.extract_batch(view)).items():
        out["host641:" + k] = v
    ctx.close()
    return out


def _check_switch_runs(oracle, res, what):
    for name in FUSED0_CASES:
        _check_vs_oracle(oracle, CASE[name], {k.split(":")[1]: v for k, v in res.items() if k.startswith(name + ":")}, what)
    par = oracle.default_params()
    for f in (0, 21, XCD_FRAMES - 1):
        c = res["xcd:counts"][f]
        _same(res["xcd:kps"][f, :c], res["xcd:desc"][f, :c], _ref(oracle, "default", 100 + f), (what, "xcd", f))
    imgs = synth.frames(200, 128)
    for f in (0, 63, 64, 127):
        c = res["host128:counts"][f]
        _same(res["host128:kps"][f, :c], res["host128:desc"][f, :c], oracle.orb_extract(par, imgs[f]), (what, "host128", f))
    for f in range(5):
        c = res["host641:counts"][f]
        _same(res["host641:kps"][f, :c], res["host641:desc"][f, :c], _ref(oracle, "init641", 30 + f), (what, "host641", f))


@pytest.fixture(scope="module")
def default_switch_runs(ctx, oracle):
    res = _switch_runs()             # (on a context of its own, like the children; ctx only brings torch up first)
    _check_switch_runs(oracle, res, "defaults")
    return res


def test_switch_geometry():
    """The 43-frame batch gives k_fast_cells and k_orient_desc item counts that are not multiples of 24 (CCM_ORB_XCD=3)."""
    ex = ORBextractor(*PSETS["default"][0])
    od, items = _od_items(ex, 752, 480, XCD_FRAMES)
    fc = _fast_bands(ex, 752, 480) * XCD_FRAMES
    assert items == 8 and od % 24 and fc % 24, (od, fc)


SWITCHES = [{"CCM_ORB_FUSED": "0"}, {"CCM_ORB_XCD": "0"}, {"CCM_ORB_XCD": "1"}, {"CCM_ORB_XCD": "3"},
            {"CCM_ORB_UPLOAD_2D": "1"}, {"CCM_ORB_CHUNK": "2"}]


@pytest.mark.parametrize("env", SWITCHES, ids=["%s=%s" % next(iter(e.items())) for e in SWITCHES])
def test_switches_change_nothing(default_switch_runs, oracle, env, tmp_path):
    """Work order (CCM_ORB_XCD 0 / 1 / chunk-cyclic 3), two-kernel FAST (CCM_ORB_FUSED=0, k_fast_score's own staging), the 2-D
    upload of a linear-capable batch (CCM_ORB_UPLOAD_2D=1) and the linear chunked upload of padded frames (CCM_ORB_CHUNK=2):
    the switches are read once per process, so each runs in a child; every byte equals the default run's and the oracle's."""
    path = str(tmp_path / "runs.npz")
    code = ("import sys, numpy as np, torch\n"            # torch before libccm_hot.so (tests/conftest.py)
            "sys.path.insert(0, %r)\n"
            "import test_caller_layouts_gpu as T\n"
            "np.savez(%r, **T._switch_runs())\n"
            "print('ok')\n" % (os.path.join(ROOT, "tests"), path))
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **env),
                         capture_output=True, text=True, timeout=330)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-3000:]
    with np.load(path) as z:
        res = {k: z[k] for k in z.files}
    _identical(res, default_switch_runs, str(env))
    _check_switch_runs(oracle, res, str(env))


# ------------------------------------------------------------------------------------------------- 4. host entry point, real strides
def test_host_shim_form(ctx, oracle):
    """What the shim passes: one image, stride = cv::Mat::step > w, image_stride = 0."""
    ex = ORBextractor(*PSETS["default"][0], ctx=ctx)
    img = _frame("default", 40)
    for stride, off in ((757, 0), (800, 3)):
        buf = _place(img[None], stride, 0, off, "random")
        view = np.lib.stride_tricks.as_strided(buf[off:], shape=(480, 752), strides=(stride, 1))
        kps, desc = ex(view)
        _same(kps, desc, _ref(oracle, "default", 40), stride)
        k2, d2 = ex(img)
        assert (kps == k2).all() and (desc == d2).all()


def test_host_plane_gap(ctx, oracle):
    """Five frames with a row stride and an odd gap between planes: the per-image copy loop of ccm_orb_extract."""
    ex = ORBextractor(*PSETS["default"][0], ctx=ctx)
    view, frames = _host_gap_view(5, 752, 480, 770, 770 * 480 + 13, 41, pset="default")
    got = ex.extract_batch(view)
    packed = ex.extract_batch(frames)
    for a, b in zip(got, packed):
        assert (a == b).all()
    for f in range(5):
        c = got[2][f]
        _same(got[0][f, :c], got[1][f, :c], _ref(oracle, "default", 41 + f), f)


# ------------------------------------------------------------------------------------------------- 5. capacity
def _d2h(ptr, nbytes):
    """Host copy of device memory the library owns (hipMemcpy of the HIP runtime libccm_hot.so is bound to)."""
    lib = _lib.load()
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.zeros(nbytes, np.uint8)
    assert lib.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0     # hipMemcpyDeviceToHost
    return out


def test_capacity_is_reported_then_clears(ctx, oracle):
    import torch
    imgs = np.stack([_frame("default", 50), _frame("default", 51), np.full((480, 752), 90, np.uint8)])    # the flat frame: 0 keypoints
    refs = [_ref(oracle, "default", 50), _ref(oracle, "default", 51), oracle.orb_extract(oracle.default_params(), imgs[2])]
    small = ORBextractor(*PSETS["default"][0], ctx=ctx, max_per_image=300)
    with pytest.raises(_lib.CcmError) as e:
        small.extract_batch(imgs)
    assert e.value.code == E_CAPACITY
    dev = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    small.extract_dev(dev.data_ptr(), 752, 480, 752, 752 * 480, 3)       # asynchronous: no error yet
    with pytest.raises(_lib.CcmError) as e:
        small.fetch()
    assert e.value.code == E_CAPACITY
    d_ptr, c_ptr, m = small.result_dev()
    assert m == 300
    ctx.sync()
    counts = _d2h(c_ptr, 12).view(np.int32)
    assert (counts == [min(len(r["kps"]), 300) for r in refs]).all() and len(refs[0]["kps"]) > 300
    desc = _d2h(d_ptr, 3 * 300 * 32).reshape(3, 300, 32)
    for f in range(2):                                                     # the rows that fit are the first ones, exact
        assert (desc[f] == refs[f]["desc"][:300]).all(), f
    # the next calls on the same context, with a proper cap: exact, no stale status word
    ex = ORBextractor(*PSETS["default"][0], ctx=ctx)
    ex.extract_dev(dev.data_ptr(), 752, 480, 752, 752 * 480, 3)
    kps, desc, counts = ex.fetch()
    for f in range(3):
        _same(kps[f, :counts[f]], desc[f, :counts[f]], refs[f], f)
    kps, desc, counts = ex.extract_batch(imgs)
    for f in range(3):
        _same(kps[f, :counts[f]], desc[f, :counts[f]], refs[f], f)


# ------------------------------------------------------------------------------------------------- 6. matcher strides, device counts
def _match_dev(ctx, q_ptr, nq, qs, t_ptr, nt, ts, n_pairs, nq_ptr, nt_ptr):
    import torch
    lib = _lib.load()
    outs = [torch.full((n_pairs, nq), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    rc = lib.ccm_hamming_match_dev(ctx.handle, C.c_void_p(q_ptr), nq, C.c_size_t(qs), C.c_void_p(t_ptr), nt, C.c_size_t(ts), n_pairs,
                                   C.c_void_p(nq_ptr), C.c_void_p(nt_ptr), *[C.c_void_p(o.data_ptr()) for o in outs])
    ctx.check(rc)
    ctx.sync()
    return [o.cpu().numpy() for o in outs]


def _check_pairs(oracle, q, t, nqn, ntn, got, what=""):
    bi, bd, sd = got
    for p in range(len(nqn)):
        a, b = int(nqn[p]), int(ntn[p])
        rbi, rbd, rsd = oracle.hamming_match(q[p][:a], t[p][:b])
        assert (bi[p, :a] == rbi).all() and (bd[p, :a] == rbd).all() and (sd[p, :a] == rsd).all(), (what, p)
        assert (bi[p, a:] == -1).all() and (bd[p, a:] == 256).all() and (sd[p, a:] == 256).all(), (what, p)


def test_bench_step_all_pairs(ctx, oracle):
    """bench.py's step: extract_dev of 256 frames, then pairs (f, f+1) read in place with pair strides of max_per_image rows and
    live counts from counts_dev.  All 255 pairs against the oracle's matcher on the oracle's descriptors."""
    import torch
    ex = ORBextractor(*PSETS["default"][0], ctx=ctx)
    imgs = synth.frames(0, 256)
    dev = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    ex.extract_dev(dev.data_ptr(), 752, 480, 752, 752 * 480, 256)
    d_ptr, c_ptr, m = ex.result_dev()
    got = _match_dev(ctx, d_ptr, m, m, d_ptr + m * 32, m, m, 255, c_ptr, c_ptr + 4)
    kps, desc, counts = ex.fetch()
    par = oracle.default_params()
    refs = [oracle.orb_extract(par, imgs[f]) for f in range(256)]
    for f in range(256):
        assert counts[f] == len(refs[f]["desc"]) and (desc[f, :counts[f]] == refs[f]["desc"]).all(), f
    rd = [r["desc"] for r in refs]
    _check_pairs(oracle, rd[:-1], rd[1:], counts[:-1], counts[1:], got, "bench step")


@pytest.mark.parametrize("nq,qs,nt,ts,n_pairs,t_shift", [
    (700, 1037, 1500, 1733, 6, None),       # matrix-core kernel (nt <= 2048), strides unlike the row counts
    (700, 1037, 2500, 2601, 3, None),       # vector-ALU kernel, few pairs: train rows split over workgroups, exact merge
    (300, 421, 2100, 2100, 150, None),      # vector-ALU kernel, many pairs
    (700, 1037, 700, 1037, 40, 5),          # t views the same buffer as q, five rows later
    (64, 64, 2048, 2111, 2, 3),             # the matrix-core kernel's largest train set
])
def test_match_dev_strides_and_counts(ctx, oracle, nq, qs, nt, ts, n_pairs, t_shift):
    """Pair strides different from the row counts, live counts on the device, random bytes in the rows past them."""
    import torch
    rng = np.random.default_rng(nq * 7 + nt)
    nqn = rng.integers(0, nq + 1, n_pairs).astype(np.int32); nqn[0] = nq
    ntn = rng.integers(0, nt + 1, n_pairs).astype(np.int32); ntn[-1] = nt; ntn[n_pairs // 2] = 0
    rows = (n_pairs - 1) * qs + nq if t_shift is None else max((n_pairs - 1) * qs + nq, t_shift + (n_pairs - 1) * ts + nt)
    qbuf = rng.integers(0, 256, (rows + 8, 32), dtype=np.uint8)
    base = synth.descriptor_pair(nq, nq)[0][:min(nq, 64)]          # some near-duplicates: distance ties and small distances
    qbuf[:len(base)] = base; qbuf[nq // 2:nq // 2 + len(base)] = base
    q = [qbuf[p * qs:p * qs + nq] for p in range(n_pairs)]
    qd = torch.from_numpy(qbuf).cuda()
    if t_shift is None:
        tbuf = rng.integers(0, 256, ((n_pairs - 1) * ts + nt + 8, 32), dtype=np.uint8)
        tbuf[3:3 + len(base)] = base ^ 1
        td = torch.from_numpy(tbuf).cuda()
        t_ptr = td.data_ptr()
        t = [tbuf[p * ts:p * ts + nt] for p in range(n_pairs)]
    else:
        t_ptr = qd.data_ptr() + 32 * t_shift
        t = [qbuf[p * ts + t_shift:p * ts + t_shift + nt] for p in range(n_pairs)]
    cn = torch.from_numpy(np.concatenate([nqn, ntn])).cuda()
    got = _match_dev(ctx, qd.data_ptr(), nq, qs, t_ptr, nt, ts, n_pairs, cn.data_ptr(), cn.data_ptr() + 4 * n_pairs)
    _check_pairs(oracle, q, t, nqn, ntn, got)
    got_all = _match_dev(ctx, qd.data_ptr(), nq, qs, t_ptr, nt, ts, n_pairs, None, None)      # NULL counts: every row live
    _check_pairs(oracle, q, t, np.full(n_pairs, nq), np.full(n_pairs, nt), got_all, "all live")


def test_match_dev_rejects_bad_arguments(ctx):
    import torch
    lib = _lib.load()
    buf = torch.zeros((70000, 32), dtype=torch.uint8, device="cuda")
    out = torch.zeros(3 * 64, dtype=torch.int32, device="cuda")
    o = [C.c_void_p(out.data_ptr() + 4 * 64 * i) for i in range(3)]
    p = buf.data_ptr()

    def call(q, nt, t):
        return lib.ccm_hamming_match_dev(ctx.handle, C.c_void_p(q), 64, C.c_size_t(64), C.c_void_p(t), nt, C.c_size_t(nt), 1, None, None, *o)
    assert call(p + 8, 100, p + 32 * 100) == E_ARG
    assert call(p, 100, p + 32 * 100 + 4) == E_ARG
    assert call(p, 65536, p + 32 * 64) == E_ARG
    assert call(p + 16, 100, p + 32 * 100 + 16) == 0                   # 16-byte aligned, not row aligned: accepted
    ctx.sync()


# ------------------------------------------------------------------------------------------------- 7. vocabulary on device descriptors
@pytest.fixture(scope="module")
def tree():
    return synthetic_tree(10, 4, seed=11, ragged=True)


def test_voc_transform_dev_on_extract_results(ctx, oracle, tree):
    """Each frame's descriptors read in place from the extractor's result buffer (same context: stream order covers the read)."""
    import torch
    par, d, w = tree
    voc = ORBVocabulary(10, 4, par, d, w, ctx=ctx)
    ref = oracle.Voc(10, 4, par, d, w)
    ex = ORBextractor(*PSETS["default"][0], ctx=ctx)
    dev = torch.from_numpy(synth.frames(60, 6)).cuda()
    torch.cuda.synchronize()
    ex.extract_dev(dev.data_ptr(), 752, 480, 752, 752 * 480, 6)
    d_ptr, _, m = ex.result_dev()
    _, desc, counts = ex.fetch()
    for f in range(6):
        n = int(counts[f])
        got = voc.transform_features_dev(d_ptr + f * m * 32, n, 3)
        host = voc.transform_features(desc[f, :n], 3)
        rr = ref.transform_features(desc[f, :n], 3)
        for a, b, c in zip(got, host, rr):
            assert len(a) == n and (a == b).all() and (a == c).all(), f


def test_voc_transform_dev_sizes(ctx, oracle, tree):
    import torch
    par, d, w = tree
    voc = ORBVocabulary(10, 4, par, d, w, ctx=ctx)
    ref = oracle.Voc(10, 4, par, d, w)
    rng = np.random.default_rng(12)
    n = 256000
    feats = d[rng.integers(1, len(par), n)] ^ np.packbits(rng.random((n, 256)) < 0.1, axis=1, bitorder="little")
    feats[::7] = rng.integers(0, 256, (len(feats[::7]), 32), dtype=np.uint8)
    fd = torch.from_numpy(feats).cuda()
    torch.cuda.synchronize()
    got = voc.transform_features_dev(fd.data_ptr(), n, 4)
    host = voc.transform_features(feats, 4)
    for a, b in zip(got, host):
        assert (a == b).all()
    sample = rng.choice(n, 20000, replace=False)
    for a, c in zip(got, ref.transform_features(feats[sample], 4)):
        assert (a[sample] == c).all()
    for k in (0, 1, 257):                                               # from a 16-byte aligned offset into the buffer
        off = 992 + 16 * (k % 2)
        sub = feats.reshape(-1)[off:off + 32 * k].reshape(k, 32)
        got = voc.transform_features_dev(fd.data_ptr() + off, k, 2)
        for a, b, c in zip(got, voc.transform_features(sub, 2), ref.transform_features(sub, 2)):
            assert len(a) == k and (a == b).all() and (a == c).all(), k
    for bad in (1, 8, 4):
        with pytest.raises(_lib.CcmError) as e:
            voc.transform_features_dev(fd.data_ptr() + bad, 10, 2)
        assert e.value.code == E_ARG
    empty = ORBVocabulary(10, 6, [0], np.zeros((1, 32), np.uint8), [0.0], ctx=ctx)
    eref = oracle.Voc(10, 6, [0], np.zeros((1, 32), np.uint8), [0.0])
    got = empty.transform_features_dev(fd.data_ptr(), 300, 2)
    for a, b, c in zip(got, empty.transform_features(feats[:300], 2), eref.transform_features(feats[:300], 2)):
        assert len(a) == 300 and (a == b).all() and (a == c).all()
    with pytest.raises(_lib.CcmError) as e:
        empty.transform_features_dev(fd.data_ptr() + 8, 300, 2)
    assert e.value.code == E_ARG
