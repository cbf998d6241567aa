"""ccm_map_table_refresh (include/ccm_hot.h "map-point table") on the CPU: declared, exported, refusing NULL arguments before it
touches a device; the Python mirror; known answers of the numpy restatement tests/map_refresh_ref.py that the GPU tests compare
against, and the conditions its scene must fulfil so that those tests cannot pass trivially.  No GPU work here."""
import ctypes as C
import os
import re

import numpy as np

import map_refresh_ref as R
import search_local_points_ref as SLP
from motioncheck_ccm_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
F = np.float32


def _desc(*bits):
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b >> 3] |= 1 << (b & 7)
    return d


def test_entry_point_declared_and_exported():
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccm_hot.h")).read(), flags=re.S)
    assert re.search(r"\bccm_map_table_refresh\s*\(", h)
    assert re.search(r"}\s*ccm_map_refresh\s*;", h) and re.search(r"}\s*ccm_map_refresh_result\s*;", h)
    assert re.search(r"\bCCM_MPR_DESCRIPTOR\s*=\s*1\b", h) and re.search(r"\bCCM_MPR_NORMAL_DEPTH\s*=\s*2\b", h)
    for field in ("slot", "pos", "flags", "n_kf", "kfs", "obs_first", "obs_kf", "obs_feat", "ref_kf", "ref_feat", "what"):
        assert field in [f[0] for f in _lib.MapRefresh._fields_], field
        assert re.search(r"\b%s\s*;" % field, h), field
    assert [f[0] for f in _lib.MapRefreshResult._fields_] == ["best", "normal", "min_dist", "max_dist"]
    lib = _lib.load()
    assert "ccm_map_table_refresh" in _lib.SYMBOLS and hasattr(lib, "ccm_map_table_refresh")
    assert lib.ccm_abi_version() == 3 == _lib.ABI_VERSION         # additions only
    assert (_lib.MPR_DESCRIPTOR, _lib.MPR_NORMAL_DEPTH) == (R.DESCRIPTOR, R.NORMAL_DEPTH) == (1, 2)


def test_null_context_table_or_problem_is_an_argument_error():
    lib = _lib.load()
    slot = np.zeros(1, "i4"); first = np.zeros(2, "i4")
    u = _lib.MapRefresh(1, _lib.ptr(slot), None, None, 0, None, _lib.ptr(first), None, None, None, None, 3)
    best = np.full(1, 77, "i4")
    r = _lib.MapRefreshResult(_lib.ptr(best), None, None, None)
    fake = C.c_void_p(8)                                          # never dereferenced: the NULL argument is found first
    assert lib.ccm_map_table_refresh(None, None, C.byref(u), C.byref(r)) == E_ARG
    assert lib.ccm_map_table_refresh(None, fake, C.byref(u), C.byref(r)) == E_ARG
    assert lib.ccm_map_table_refresh(fake, None, C.byref(u), C.byref(r)) == E_ARG
    assert lib.ccm_map_table_refresh(None, None, None, None) == E_ARG
    u0 = _lib.MapRefresh(1, None, None, None, 0, None, None, None, None, None, None, 3)   # no arrays at all
    assert lib.ccm_map_table_refresh(None, None, C.byref(u0), None) == E_ARG
    assert best[0] == 77


def test_python_mirror_is_exposed():
    from motioncheck_ccm_slam_amd import tracking
    assert callable(tracking.MapPointTable.refresh)
    assert (tracking.MPR_DESCRIPTOR, tracking.MPR_NORMAL_DEPTH) == (1, 2)
    import inspect
    sig = inspect.signature(tracking.MapPointTable.refresh)
    assert list(sig.parameters)[1:] == ["slot", "kfs", "obs_first", "obs_kf", "obs_feat", "ref_kf", "ref_feat", "pos", "flags", "what", "fetch"]
    assert sig.parameters["what"].default == 3 and sig.parameters["fetch"].default is True


# ------------------------------------------------------------------------------------------------------------ known answers
def test_one_observation_on_the_axis():
    sf = R.SCALE
    assert sf[2] == F(F(1.2) * F(1.2))                            # 1.44f
    n, mn, mx = R.normal_depth([0, 0, 4], [[0, 0, 0]], [0, 0, 0], 2)
    assert (n.view("u4") == np.array([0, 0, 1], "f4").view("u4")).all()
    assert mx == F(4) * sf[2] and mn == F(mx / sf[7])
    assert F(mx).view("u4") == F(F(4) * F(F(1.2) * F(1.2))).view("u4")
    n, _, _ = R.normal_depth([0, 0, 0], [[0, 0, -3], [0, 0, 5]], [0, 0, -3], 0)   # seen from opposite sides
    assert (n == 0).all()


def test_mean_of_three_multiplies_by_the_reciprocal():
    """Mat / 3 is normal * (float)(1.0 / 3), which differs from a float division for some sums."""
    P = np.array([0.3, -0.2, 0.1], "f4")
    Ows = np.array([[1, 0.5, -4], [-0.7, 0.2, -3.5], [0.1, -0.9, -4.4]], "f4")
    s = R.ray_sum(P, Ows)
    by_mul, by_div = s * F(1.0 / 3.0), s / F(3)
    assert (by_mul.view("u4") != by_div.view("u4")).any()
    n, _, _ = R.normal_depth(P, Ows, Ows[0], 0)
    assert (n.view("u4") == by_mul.view("u4")).all()
    # each addend is rounded as a product before it is added: the sum of one observation is the rounded product itself
    d = P - Ows[0]
    a = F(1.0 / np.sqrt((np.float64(d[0]) * d[0] + np.float64(d[1]) * d[1]) + np.float64(d[2]) * d[2]))
    assert (R.ray_sum(P, Ows[:1]).view("u4") == (d * a).astype("f4").view("u4")).all()


def test_descriptor_choice_known_answers(oracle):
    d = np.stack([_desc(0, 1), _desc(), _desc(2, 3, 4, 5)])       # the tie case of tests/test_bow_cpu.py: medians 2, 2, 4
    assert R.distinctive(d) == (0, True) and R.distinctive(d[[2, 1, 0]]) == (1, True)
    assert R.distinctive(d[:1]) == (0, False) and R.distinctive(d[:0]) == (-1, False)
    S = R.scene(1)
    g, first, count = R.gathered_descriptors(S)
    ref = R.refresh(S, {k: v[S["slot"]] for k, v in R.table_rows(2).items()}, R.DESCRIPTOR)
    for p in range(len(count)):
        if count[p]:
            assert ref["best"][p] == oracle.distinctive_descriptor(g[first[p]:first[p] + count[p]]), p
            assert (ref["desc"][p] == g[first[p] + ref["best"][p]]).all()
        else:
            assert ref["best"][p] == -1


# ------------------------------------------------------------------------------------------------------------ scene
def test_scene_conditions():
    S = R.scene(1)
    before = {k: v[S["slot"]] for k, v in R.table_rows(2).items()}
    ref = R.refresh(S, before, 3, pos=S["pos"])
    c = S["counts"]
    assert len(S["kfs"]) == 8 and all(len(k["desc"]) == 300 for k in S["kfs"]) and len(c) == 400
    assert len(np.unique(S["slot"])) == 400 and S["slot"].max() < R.CAPACITY
    for want in R.COUNTS:
        assert (c == want).any(), want
    assert c.max() > 256                                          # above the kernel's LDS budget
    many = c >= 3
    print("ties: %d of %d points with c >= 3" % (ref["tie"][many].sum(), many.sum()))
    assert ref["tie"][many].sum() >= 0.2 * many.sum()
    nan = np.isnan(ref["normal"]).any(1) | np.isnan(ref["min_dist"]) | np.isnan(ref["max_dist"])
    assert nan.sum() == 1 and nan[S["on_centre"]]
    ref_oct = np.array([S["kfs"][k]["oct"][f] for k, f in zip(S["ref_kf"], S["ref_feat"])])
    assert ref_oct[S["octave0"]] == 0 and ref_oct[S["octave7"]] == 7 and c[S["octave0"]] > 0 and c[S["octave7"]] > 0
    outside = [p for p in range(400) if c[p] and not ((S["obs_kf"][S["obs_first"][p]:S["obs_first"][p + 1]] == S["ref_kf"][p]) &
                                                        (S["obs_feat"][S["obs_first"][p]:S["obs_first"][p + 1]] == S["ref_feat"][p])).any()]
    assert len(outside) >= 10                                     # reference keyframes that are not in the list
    worst = 0.0
    for p in range(400):
        a, b = S["obs_first"][p], S["obs_first"][p + 1]
        if a == b:                                                # the row stays
            assert (ref["normal"][p].view("u4") == before["normal"][p].view("u4")).all() and (ref["desc"][p] == before["desc"][p]).all()
            continue
        Ows = np.stack([S["kfs"][k]["Ow"] for k in S["obs_kf"][a:b]])
        if p != S["on_centre"]:
            dist = np.linalg.norm(S["pos"][p].astype("f8") - Ows.astype("f8"), axis=1)
            assert (dist >= 2).all() and (dist <= 6).all()
            err = np.abs(ref["normal"][p].astype("f8") - R.normal_depth64(S["pos"][p], Ows)).max()
            assert err <= (c[p] + 3) * 2.0 ** -23, (p, c[p], err)
            worst = max(worst, err / ((c[p] + 3) * 2.0 ** -23))
    print("worst float32 error of the normal: %.2f of its bound" % worst)
    # the downstream test looks at the refreshed rows through a camera in front of the cloud: most of them must be in view
    sub = np.flatnonzero((c > 0) & ~nan)[:200]
    rows = dict(pos=S["pos"][sub], normal=ref["normal"][sub], min_dist=ref["min_dist"][sub], max_dist=ref["max_dist"][sub])
    fr = SLP.frustum(rows["pos"], rows["normal"], rows["min_dist"], rows["max_dist"], *downstream_camera())
    print("downstream: %d of 200 in view" % (fr["gate"] == 0).sum())
    assert (fr["gate"] == 0).sum() >= 100


def test_batched_normal_equals_the_point_by_point_one():
    """tools/bench_map_refresh.py times the vectorised form as the old route's host step; it must be the same arithmetic."""
    S = R.scene(1)
    ref = R.refresh(S, {k: v[S["slot"]] for k, v in R.table_rows(2).items()}, R.NORMAL_DEPTH, pos=S["pos"])
    kfs = S["kfs"]
    lvl = np.array([kfs[k]["oct"][f] for k, f in zip(S["ref_kf"], S["ref_feat"])])
    n, mn, mx = R.normal_depth_batch(S["pos"], np.stack([k["Ow"] for k in kfs]), S["obs_first"], S["obs_kf"],
                                     np.stack([kfs[k]["Ow"] for k in S["ref_kf"]]), R.SCALE[lvl], np.full(len(lvl), R.SCALE[-1]))
    has = (S["counts"] > 0) & (np.arange(len(lvl)) != S["on_centre"])
    assert (n[has].view("u4") == ref["normal"][has].view("u4")).all()
    assert (mn[has].view("u4") == ref["min_dist"][has].view("u4")).all() and (mx[has].view("u4") == ref["max_dist"][has].view("u4")).all()
    assert np.isnan(n[S["on_centre"]]).any()


def downstream_camera():
    return SLP.camera(rotvec=(0.03, -0.05, 0.02), t=(0.0, 0.0, 4.0))
