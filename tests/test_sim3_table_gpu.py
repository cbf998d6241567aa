"""ccm_search_by_sim3_table_frames on the GPU: gate, u and v of both directions against the numpy restatement tests/sim3_table_ref.py
bit for bit, the level equal except on entries the restatement flags as ambiguous (within 1 there), and sel1 / sel2 / match12 / n_found
byte for byte against tests/window_matcher_ref.py and against the array route -- ccm_search_by_sim3 fed the restatement's arrays.
Every wave and workgroup boundary of the compaction and of the agreement kernel, entry marks, BAD and not-LIVE slots, one handle on
both sides, scales, unequal intrinsics, shared keyframes, determinism, stream order and misuse."""
import ctypes as C

import numpy as np
import pytest

import fuse_table_ref as R
import sim3_table_ref as Q
from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher
from motioncheck_ccm_slam_amd.orb import ORBextractor
from motioncheck_ccm_slam_amd.tracking import MapPointTable

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -7
TAPS = ("gate", "u", "v", "level", "sel")
TH = 7.5


def _bits(a):
    return np.ascontiguousarray(a, "f4").view("u4")


def _view(kf):
    b = kf.get("bounds", Q.BOUNDS)
    return FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"].reshape(-1, 32), b[0], b[1], b[2], b[3])


class Handles:
    """One DeviceFrame per keyframe dict of a scene."""

    def __init__(self, ctx, sc):
        self.h = {}
        for kf in sc["kfs"]:
            h = DeviceFrame(_view(kf), None, ctx=ctx)
            h.map_points = kf["mp_id"]
            self.h[id(kf)] = h

    def __getitem__(self, kf):
        return self.h[id(kf)]

    def close(self):
        for h in self.h.values():
            h.close()


def _table(ctx, sc):
    t = MapPointTable(sc["capacity"], ctx=ctx)
    live = np.flatnonzero(sc["rows"]["flags"] & R.LIVE)
    if len(live):
        t.update(live, **{k: sc["rows"][k][live] for k in R.COLS})
    return t


def _call(m, t, hs, sc, pairs=None, taps=True):
    pairs = sc["pairs"] if pairs is None else pairs
    return m.SearchBySim3TableFrames(t, [dict(p, kf1=hs[p["kf1"]], kf2=hs[p["kf2"]]) for p in pairs], Q.SCALE, th=TH, log_scale_factor1=Q.LOG_SF,
                                     taps=taps)


def _check(m, res, sc, pairs=None):
    """res against the restatement, the independent matcher and the array route.  Returns per pair (d1, d2, n_found)."""
    pairs = sc["pairs"] if pairs is None else pairs
    out = []
    total = 0
    for k, p in enumerate(pairs):
        ds = Q.sim3_pair(sc, p)
        levels = []
        for d, g in zip("12", ds):
            gate, lvl = res["gate" + d][k], res["level" + d][k]
            assert (gate == g["gate"]).all(), (k, d, np.flatnonzero(gate != g["gate"])[:10])
            early = (g["gate"] >= Q.NO_POINT) & (g["gate"] <= Q.BEHIND)            # rejected before the projection: the taps hold 0
            for c in ("u", "v"):
                got, want = res[c + d][k], g[c]
                cmp = ~early & ~np.isnan(want)                                      # a NaN's sign bit is not fixed
                assert (_bits(got)[cmp] == _bits(want)[cmp]).all(), (k, c + d)
                assert np.isnan(got[~early & np.isnan(want)]).all() and (_bits(got)[early] == 0).all(), (k, c + d)
            diff = lvl - g["level"]
            amb = g["ambiguous"]
            assert (diff[~amb] == 0).all() and (np.abs(diff[amb]) <= 1).all(), (k, d)
            levels.append(np.where(amb, lvl, g["level"]))                           # the device's level where both are valid
        d1, d2 = ds
        found, m12, sel1, sel2 = Q.sim3_select(p, d1, d2, levels[0], levels[1], TH)
        assert res["sel1"][k].tobytes() == sel1.tobytes() and res["sel2"][k].tobytes() == sel2.tobytes(), k
        assert res["match12"][k].tobytes() == m12.tobytes() and res["n_found"][k] == found, k
        k1, k2 = p["kf1"], p["kf2"]
        if len(k1["kx"]) and len(k2["kx"]):                                         # the array route on the restatement's arrays
            n, a12 = m.SearchBySim3(_view(k1), Q.SCALE, _view(k2), Q.SCALE, d1["gate"] == Q.SEARCHED, d1["u"], d1["v"], levels[0], d1["desc"],
                                    d2["gate"] == Q.SEARCHED, d2["u"], d2["v"], levels[1], d2["desc"], TH)
            assert res["match12"][k].tobytes() == a12.tobytes() and n == found, k
            for sel, src, dst, d, lv in ((sel1, k1, k2, d1, levels[0]), (sel2, k2, k1, d2, levels[1])):
                bi, _ = m.FuseSelect(_view(dst), Q.SCALE, R.INV_SIGMA2, d["gate"] == Q.SEARCHED, d["u"], d["v"], lv, d["desc"], TH, False, 100)
                assert sel.tobytes() == bi.tobytes(), k
        total += found
        out.append((d1, d2, found))
    assert res["total"] == total
    return out


@pytest.fixture(scope="module")
def feat(ctx):
    kps, desc = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)(synth.frame(1))
    assert len(kps) >= 600
    return dict(kx=kps["x"].astype("f4"), ky=kps["y"].astype("f4"), oct=kps["octave"].astype("i4"), desc=desc)


def _run(ctx, sc, pairs=None):
    m = ORBmatcher(ctx=ctx)
    hs = Handles(ctx, sc)
    with _table(ctx, sc) as t:
        res = _call(m, t, hs, sc, pairs)
        out = _check(m, res, sc, pairs)
    hs.close()
    return res, out


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("n1,n2,n_pairs", Q.SIM3_CASES)
def test_every_compaction_and_agreement_boundary(ctx, feat, n1, n2, n_pairs):
    sc = Q.sim3_scene(feat, n1, n2, n_pairs)
    res, out = _run(ctx, sc)
    gates = sum(np.bincount(d["gate"], minlength=8) for o in out for d in o[:2])
    print("%d x %d x %d: gates %s, found %s" % (n_pairs, n1, n2, gates.tolist(), [o[2] for o in out]))
    if min(n1, n2) >= 255:
        assert all(o[2] >= 5 for o in out)
    if n_pairs >= 2:
        assert sc["pairs"][0]["kf1"] is sc["pairs"][1]["kf1"]                       # two pairs share kf1


@pytest.mark.parametrize("s12", [0.5, 1.0, 2.0])
def test_scales_and_entry_marks(ctx, feat, s12):
    sc = Q.Sim3Scene(int(10 * s12))
    kf1 = sc.keyframe(Q.cuts(feat, 500, 1), R.CAMERAS[0])
    p = sc.pair(kf1, 400, R.CAMERAS[1], s12, Q.cuts(feat, 400, 2), n_marked=40)
    sc = sc.finish()
    a1, a2 = Q.marks(p)
    assert a1.sum() == 40 and 3 <= a2.sum() < 40 and (p["matched_idx2"][a1] >= 400).any() and (p["matched_idx2"][a1] < 0).any()
    res, out = _run(ctx, sc)
    d1, d2, found = out[0]
    assert (d1["gate"] == Q.MATCHED).sum() >= 10 and (d2["gate"] == Q.MATCHED).sum() >= 1
    assert (d1["gate"] == Q.IS_BAD).sum() >= 1 and (d1["gate"] == Q.NO_POINT).sum() >= 100
    print("s12 = %g: found %d, gates %s | %s" % (s12, found, np.bincount(d1["gate"], minlength=8).tolist(), np.bincount(d2["gate"], minlength=8).tolist()))
    if s12 == 1.0:
        assert found >= 20
    else:
        assert (d1["gate"] == Q.DISTANCE).sum() >= 1


def test_one_handle_on_both_sides_and_an_empty_side(ctx, feat):
    sc = Q.Sim3Scene(4)
    kf = sc.keyframe(Q.cuts(feat, 300, 4), R.CAMERAS[0], frac=0.7)
    p = sc.pair(kf, 300, None, 1.0, None, kf2=kf)
    p["S12"] = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype("f4"); p["S21"] = p["S12"].copy()
    empty = sc.keyframe(Q.cuts(feat, 0, 5), R.CAMERAS[1])
    sc.pair(kf, 0, None, 1.0, None, kf2=empty)
    sc.pair(empty, 0, None, 1.0, None, kf2=kf)
    sc = sc.finish()
    res, out = _run(ctx, sc)
    assert out[0][2] >= 20 and out[1][2] == 0 and out[2][2] == 0
    assert (out[1][0]["gate"] == Q.EMPTY_KF).sum() >= 50 and not (out[1][0]["gate"] == Q.SEARCHED).any()


def test_unequal_intrinsics_and_bounds(ctx, feat):
    sc = Q.Sim3Scene(6)
    kf1 = sc.keyframe(Q.cuts(feat, 257, 6), R.CAMERAS[0], intr=(440.0, 450.0, 350.0, 240.0))
    inside = np.flatnonzero((feat["kx"] > 30) & (feat["kx"] < 690) & (feat["ky"] > 20) & (feat["ky"] < 450))   # the second keyframe's image is smaller
    p = sc.pair(kf1, 256, R.CAMERAS[2], 1.0, R.cut(feat, inside[:256]), intr=(440.0, 450.0, 350.0, 240.0), bounds2=(20.0, 700.0, 10.0, 460.0))
    p["kf2"]["bounds"] = p["bounds2"]
    p["intr2"] = Q.INTR                                                             # the second keyframe's own camera: never read
    sc = sc.finish()
    res, out = _run(ctx, sc)
    d1, d2, found = out[0]
    assert found >= 5 and (d1["gate"] == Q.OUTSIDE).sum() >= 1
    q = dict(p, intr=Q.INTR)                                                        # and the intrinsics matter
    e1, _ = Q.sim3_pair(sc, q)
    s = (d1["gate"] == Q.SEARCHED) & (e1["gate"] == Q.SEARCHED)
    assert s.sum() >= 10 and (e1["u"][s] != d1["u"][s]).all()


def test_three_pairs_twice_give_equal_bytes_with_and_without_taps(ctx, feat):
    sc = Q.sim3_scene(feat, 257, 256, 3, seed=23)
    m = ORBmatcher(ctx=ctx)
    hs = Handles(ctx, sc)
    with _table(ctx, sc) as t:
        a = _call(m, t, hs, sc)
        _check(m, a, sc)
        b = _call(m, t, hs, sc)
        plain = _call(m, t, hs, sc, taps=False)
        for k in range(3):
            for key in ("match12",) + tuple(x + d for x in TAPS for d in "12"):
                assert a[key][k].tobytes() == b[key][k].tobytes(), (key, k)         # the order of the query list is free, the outputs are not
            assert plain["match12"][k].tobytes() == a["match12"][k].tobytes()
        assert plain["n_found"] == a["n_found"] and "gate1" not in plain
        one = _call(m, t, hs, sc, pairs=sc["pairs"][1:2])                           # a pair alone gives what it gives in the batch
        assert one["match12"][0].tobytes() == a["match12"][1].tobytes()
    hs.close()


def test_sees_updates_queued_just_before(ctx, feat):
    sc = Q.sim3_scene(feat, 256, 257, 1, seed=31)
    m = ORBmatcher(ctx=ctx)
    hs = Handles(ctx, sc)
    p = sc["pairs"][0]
    rng = np.random.default_rng(2)
    with _table(ctx, sc) as t:
        first = _call(m, t, hs, sc)
        d1, d2, found = _check(m, first, sc)[0]
        s1 = np.flatnonzero(d1["gate"] == Q.SEARCHED)
        assert len(s1) >= 40
        ids = p["kf1"]["mp_id"]
        moved = ids[s1[:20]]
        sc["rows"]["pos"][moved] += rng.normal(0, 0.02, (20, 3)).astype("f4")
        sc["rows"]["flags"][ids[s1[20:30]]] |= R.BAD
        new_ids = ids.copy(); new_ids[s1[30:40]] = -1
        p["kf1"]["mp_id"] = new_ids
        t.update(moved, pos=sc["rows"]["pos"][moved])                               # no synchronisation between these and the call
        t.update(ids[s1[20:30]], flags=sc["rows"]["flags"][ids[s1[20:30]]])
        hs[p["kf1"]].map_points = new_ids
        res = _call(m, t, hs, sc)
        e1, _, _ = _check(m, res, sc)[0]
        assert (e1["gate"][s1[20:30]] == Q.IS_BAD).all() and (e1["gate"][s1[30:40]] == Q.NO_POINT).all()
        assert (_bits(e1["u"][s1[:20]]) != _bits(d1["u"][s1[:20]])).any()
    hs.close()


# ---------------------------------------------------------------------------------------------------------------- misuse
def _raw(ctx, table, h1, h2, n1, n_levels=Q.N_LEVELS, drop=(), only_u=False, n_pairs=1):
    """The C call on one pair with sentinel-filled outputs.  Returns (rc, outputs untouched)."""
    lib = _lib.load()
    rec = (_lib.Sim3SearchPair * 1)()
    I = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    rec[0].kf1 = h1; rec[0].kf2 = h2
    for name in ("T1w", "T2w", "S21", "S12"):
        getattr(rec[0], name)[:] = [float(x) for x in I]
    rec[0].fx, rec[0].fy, rec[0].cx, rec[0].cy = Q.INTR
    rec[0].bounds1[:] = Q.BOUNDS; rec[0].bounds2[:] = Q.BOUNDS
    none = np.full(max(n1, 1), -1, "i4")
    rec[0].matched12 = None if "matched12" in drop else _lib.ptr(none)
    rec[0].matched_idx2 = None if "matched_idx2" in drop else _lib.ptr(none)
    prob = _lib.Sim3SearchProblem(n_pairs, None if "pairs" in drop else rec, TH, float(Q.LOG_SF), n_levels, None if "sf" in drop else _lib.ptr(Q.SCALE),
                                  float(Q.LOG_SF), Q.N_LEVELS, _lib.ptr(Q.SCALE))
    n = 1024
    out = dict(match12=np.full(n, 12345, "i4"), n_found=np.full(4, 12345, "i4"), u1=np.full(n, 7.5, "f4"), v1=np.full(n, 7.5, "f4"),
               level1=np.full(n, 12345, "i4"))
    g = lambda k: None if k in drop or (only_u and k in ("v1", "level1")) else _lib.ptr(out[k])  # noqa: E731
    res = _lib.Sim3SearchResult(g("match12"), g("n_found"), None, g("u1"), g("v1"), g("level1"), None, None, None, None, None, None)
    rc = lib.ccm_search_by_sim3_table_frames(ctx.handle, C.c_void_p(table), C.byref(prob), C.byref(res))
    untouched = all((out[k] == (7.5 if k in ("u1", "v1") else 12345)).all() for k in out)
    return rc, untouched


def test_misuse_returns_error_codes_and_leaves_the_outputs(ctx, feat):
    sc = Q.sim3_scene(feat, 65, 64, 1)
    hs = Handles(ctx, sc)
    p = sc["pairs"][0]
    h1, h2 = hs[p["kf1"]].handle, hs[p["kf2"]].handle
    other = _lib.Context(0)
    try:
        with _table(ctx, sc) as t:
            rc, untouched = _raw(ctx, t.handle, h1, h2, 65)
            assert rc >= 0 and not untouched                                         # the well-formed call runs
            for drop in (("pairs",), ("sf",), ("n_found",), ("match12",), ("matched12",), ("matched_idx2",)):
                assert _raw(ctx, t.handle, h1, h2, 65, drop=drop) == (E_ARG, True), drop
            assert _raw(ctx, t.handle, h1, h2, 65, only_u=True) == (E_ARG, True)     # only some of u / v / level
            assert _raw(ctx, t.handle, h1, h2, 65, n_levels=0) == (E_ARG, True)
            assert _raw(ctx, t.handle, h1, h2, 65, n_levels=17) == (E_ARG, True)
            assert _raw(ctx, t.handle, h1, None, 65) == (E_ARG, True)                # a pair without a handle
            assert _raw(ctx, t.handle, h1, h2, 65, n_pairs=-1) == (E_ARG, True)
            assert _raw(ctx, t.handle, h1, h2, 65, n_pairs=0) == (0, True)           # zero pairs: CCM_OK, nothing written
            with DeviceFrame(_view(p["kf1"]), None, ctx=other) as fo, MapPointTable(sc["capacity"], ctx=other) as to:
                assert _raw(ctx, t.handle, h1, fo.handle, 65) == (E_ARG, True)       # a handle of another context
                assert _raw(ctx, to.handle, h1, h2, 65) == (E_ARG, True)             # a table of another context
                assert _raw(other, t.handle, fo.handle, fo.handle, 65) == (E_ARG, True)
            m = ORBmatcher(ctx=ctx)
            _check(m, _call(m, t, hs, sc), sc)                                       # and the context still works
        orphan_t = MapPointTable(10, ctx=other)
        orphan_f = DeviceFrame(_view(p["kf1"]), None, ctx=other)
    finally:
        other.close()
    with _table(ctx, sc) as t:                                                       # the other context is gone
        assert _raw(ctx, orphan_t.handle, h1, h2, 65) == (E_STATE, True)
        assert _raw(ctx, t.handle, h1, orphan_f.handle, 65) == (E_STATE, True)
    orphan_t.close(); orphan_f.close()
    hs.close()
