"""ccm_search_by_projection_table_frames on the GPU: gate, u and v against the numpy restatement (tests/sim3_table_ref.py, which takes
Fuse's gates from tests/fuse_table_ref.py) bit for bit, the level equal except on ambiguous pairs, and best_idx / observed /
matched_slot / n_matches byte for byte against tests/window_matcher_ref.py and against the array route
ccm_search_by_projection_sim3_batch fed the restatement's arrays.  Sizes around every block edge, the order-dependent acceptance on
hand-built cases, determinism, stream order and misuse."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fuse_table_ref as R
import search_local_points_ref as S
import sim3_table_ref as Q
from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher
from motioncheck_ccm_slam_amd.orb import ORBextractor
from motioncheck_ccm_slam_amd.tracking import MapPointTable

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -7
TH = 10.0
OUT = ("best_idx", "observed", "gate", "u", "v", "level", "best_dist")


def _bits(a):
    return np.ascontiguousarray(a, "f4").view("u4")


def _view(kf):
    return FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"].reshape(-1, 32))


def _handles(ctx, sc):
    hs = []
    for kf in sc["kfs"]:
        h = DeviceFrame(_view(kf), None, ctx=ctx)
        h.map_points = kf["mp_id"]
        hs.append(h)
    return hs


def _table(ctx, sc):
    t = MapPointTable(sc["capacity"], ctx=ctx)
    live = np.flatnonzero(sc["rows"]["flags"] & R.LIVE)
    if len(live):
        t.update(live, **{k: sc["rows"][k][live] for k in R.COLS})
    return t


def _call(m, t, hs, sc, taps=True):
    kfs = sc["kfs"]
    return m.SearchByProjectionTableFrames(t, hs, [k["Tcw"] for k in kfs], [k["Ow"] for k in kfs], [k.get("intr", R.INTR) for k in kfs],
                                           [k.get("bounds", R.BOUNDS) for k in kfs], sc["slots"], [k["matched_slot"] for k in kfs], Q.SCALE, th=TH,
                                           log_scale_factor=Q.LOG_SF, taps=taps)


def _check(m, res, sc):
    """res against the restatement, the independent matcher and the array route.  Returns (restatement, n_matches)."""
    g = Q.loop_views(sc)
    K, n = g["gate"].shape
    assert (res["gate"] == g["gate"]).all(), np.flatnonzero(res["gate"] != g["gate"])[:10]
    assert res["observed"].tobytes() == g["observed"].tobytes()
    searched = g["gate"] == Q.LG_SEARCHED
    early = (g["gate"] >= Q.LG_SKIPPED) & (g["gate"] <= Q.LG_BEHIND)                # rejected before the projection: the taps hold 0
    for k in ("u", "v"):
        cmp = ~early & ~np.isnan(g[k])                                              # a NaN's sign bit is not fixed
        assert (_bits(res[k])[cmp] == _bits(g[k])[cmp]).all(), k
        assert np.isnan(res[k][~early & np.isnan(g[k])]).all() and (_bits(res[k])[early] == 0).all(), k
    d = res["level"] - g["level"]
    amb = g["ambiguous"]
    assert (d[~amb] == 0).all() and (np.abs(d[amb]) <= 1).all()
    level = np.where(amb, res["level"], g["level"])
    nm, bi, ms = Q.loop_accept(sc, g, level, TH)
    assert res["best_idx"].tobytes() == bi.astype("i4").tobytes() and res["n_matches"].tobytes() == nm.tobytes() and res["total"] == nm.sum()
    desc = sc["rows"]["desc"][sc["slots"]]
    for k, kf in enumerate(sc["kfs"]):
        assert res["matched_slot"][k].tobytes() == ms[k].tobytes(), k
        acc = np.flatnonzero(bi[k] >= 0)                                            # the distance tap: to the chosen feature, 256 elsewhere
        want = np.full(n, 256, "i4")
        want[acc] = np.unpackbits(kf["desc"][bi[k][acc]] ^ desc[acc], axis=1).sum(1)
        assert res["best_dist"][k].tobytes() == want.tobytes() and (want[acc] <= 50).all(), k
    if n and all(len(kf["kx"]) for kf in sc["kfs"]):                                # the array route on the restatement's arrays
        arr = m.SearchByProjectionSim3Batch([_view(kf) for kf in sc["kfs"]], Q.SCALE,
                                            [(searched[k], g["u"][k], g["v"][k], level[k], desc, g["observed"][k], sc["kfs"][k]["matched_slot"] >= 0)
                                             for k in range(K)], TH)
        for k, (an, ab, am) in enumerate(arr):
            assert an == nm[k] and res["best_idx"][k].tobytes() == ab.tobytes(), k
            assert ((res["matched_slot"][k] >= 0).astype(np.uint8)).tobytes() == am.tobytes(), k
    return g, nm


@pytest.fixture(scope="module")
def feat(ctx):
    kps, desc = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)(synth.frame(1))
    assert len(kps) >= 600
    return dict(kx=kps["x"].astype("f4"), ky=kps["y"].astype("f4"), oct=kps["octave"].astype("i4"), desc=desc)


def _run(ctx, sc):
    m = ORBmatcher(ctx=ctx)
    hs = _handles(ctx, sc)
    with _table(ctx, sc) as t:
        res = _call(m, t, hs, sc)
        g, nm = _check(m, res, sc)
    for h in hs:
        h.close()
    return res, g, nm


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("n_kf", [1, 2, 3])
@pytest.mark.parametrize("n_points", [0, 1, 63, 64, 65, 257, 1025])
def test_every_block_edge(ctx, feat, n_points, n_kf):
    sc = Q.loop_scene(feat, n_points, n_kf)
    res, g, nm = _run(ctx, sc)
    print("%d x %d: gates %s, matches %s" % (n_kf, n_points, np.bincount(g["gate"].ravel(), minlength=8).tolist(), nm.tolist()))
    if n_points == 0:
        for k, kf in enumerate(sc["kfs"]):
            assert res["matched_slot"][k].tobytes() == kf["matched_slot"].tobytes() and res["total"] == 0      # vpMatched passes through
    if n_points >= 255:
        assert (nm >= 5).all() and (g["gate"] == Q.LG_ALREADY_FOUND).sum() >= n_kf
        assert ((res["best_idx"] >= 0) & (res["observed"] == 1)).sum() >= 1             # remaps: accepted, not counted


def test_thousand_features_four_thousand_points_twice(ctx):
    sc = Q.big_loop_scene()
    m = ORBmatcher(ctx=ctx)
    hs = _handles(ctx, sc)
    with _table(ctx, sc) as t:
        a = _call(m, t, hs, sc)
        g, nm = _check(m, a, sc)
        b = _call(m, t, hs, sc)
        plain = _call(m, t, hs, sc, taps=False)
        for k in OUT:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert plain["best_idx"].tobytes() == a["best_idx"].tobytes() and plain["matched_slot"][0].tobytes() == a["matched_slot"][0].tobytes()
    print("gates %s, matches %d" % (np.bincount(g["gate"].ravel(), minlength=8).tolist(), nm[0]))
    fl = sc["rows"]["flags"][sc["slots"][:20]]                   # the twenty points in vpMatched on entry: found unless skipped first
    found = int((((fl & R.LIVE) != 0) & ((fl & R.BAD) == 0)).sum())
    assert nm[0] >= 100 and found >= 10 and (g["gate"] == Q.LG_ALREADY_FOUND).sum() == found
    hs[0].close()


def test_empty_keyframe_and_one_handle_in_two_views(ctx, feat):
    sc = Q.loop_scene(feat, 300, 3)
    empty = dict(kx=np.zeros(0, "f4"), ky=np.zeros(0, "f4"), oct=np.zeros(0, "i4"), desc=np.zeros((0, 32), np.uint8))
    sc["kfs"][1].update(empty, mp_id=np.zeros(0, "i4"), matched_slot=np.zeros(0, "i4"))
    sc["kfs"][2].update({k: sc["kfs"][0][k] for k in ("kx", "ky", "oct", "desc", "mp_id")})     # view 2 = keyframe 0 under another pose,
    sc["kfs"][2]["matched_slot"] = np.full(64, -1, "i4")                                        # with a vpMatched of its own
    m = ORBmatcher(ctx=ctx)
    h0, he = _handles(ctx, dict(kfs=sc["kfs"][:2]))
    with _table(ctx, sc) as t:
        res = _call(m, t, [h0, he, h0], sc)
        g, nm = _check(m, res, sc)
    assert (g["gate"][1] == Q.LG_EMPTY_KF).sum() >= 50 and nm[1] == 0 and (res["best_idx"][1] == -1).all()
    assert nm[0] >= 5 and (g["gate"][0] != g["gate"][2]).any() and (res["observed"][0] == res["observed"][2]).all()
    h0.close(); he.close()
    none = Q.loop_scene(feat, 65, 2, n_feat=0)                                                   # no view has a feature
    res, g, nm = _run(ctx, none)
    assert res["total"] == 0 and np.isin(g["gate"], (Q.LG_SKIPPED, Q.LG_BEHIND, Q.LG_OUTSIDE, Q.LG_DISTANCE, Q.LG_ANGLE, Q.LG_EMPTY_KF)).all()


# ---------------------------------------------------------------------------------------------------------------- order
def test_hand_built_order_cases(ctx):
    feats, pts = Q.HAND_SHARED
    # two points whose windows share their nearest feature: the first in the list takes it, the second has nothing left within TH_LOW
    res, g, nm = _run(ctx, Q.hand_scene(feats, pts))
    assert res["best_idx"][0].tolist() == [0, -1] and nm[0] == 1 and res["matched_slot"][0].tolist() == [0, -1]
    # swapping the list swaps the result: now the other point owns feature 0, and this one takes its next best
    res, g, nm = _run(ctx, Q.hand_scene(feats, pts[::-1]))
    assert res["best_idx"][0].tolist() == [0, 1] and nm[0] == 2 and res["matched_slot"][0].tolist() == [0, 1]
    assert res["best_dist"][0].tolist() == [1, 49]
    # a point already in matched_slot is skipped, and its feature stays taken
    res, g, nm = _run(ctx, Q.hand_scene(feats, pts, matched_slot=[1, -1]))
    assert g["gate"][0].tolist() == [Q.LG_SEARCHED, Q.LG_ALREADY_FOUND] and res["best_idx"][0].tolist() == [1, -1]
    assert res["matched_slot"][0].tolist() == [1, 0] and nm[0] == 1
    # an observed point is accepted but neither marks nor counts, so the later point can take the same feature
    res, g, nm = _run(ctx, Q.hand_scene(feats, pts, held=[(1, 0)]))
    assert res["observed"][0].tolist() == [1, 0] and res["best_idx"][0].tolist() == [0, 0] and nm[0] == 1
    assert res["matched_slot"][0].tolist() == [1, -1]
    # a distance of exactly TH_LOW is accepted, one more is not
    res, g, nm = _run(ctx, Q.hand_scene([(300.0, 200.0, 2, 0), (500.0, 300.0, 2, 0)], [(300.0, 200.0, 2, 50), (500.0, 300.0, 2, 51)]))
    assert res["best_idx"][0].tolist() == [0, -1] and nm[0] == 1 and res["best_dist"][0].tolist() == [50, 256]
    # of two equal features the first in GetFeaturesInArea's order wins, and the level window is level - 1 .. level
    res, g, nm = _run(ctx, Q.hand_scene([(300.0, 200.0, 4, 0), (301.0, 200.0, 2, 7), (299.0, 200.0, 1, 7), (300.0, 201.0, 0, 0)], [(300.0, 200.5, 2, 7)]))
    assert res["best_idx"][0].tolist() in ([1], [2]) and res["best_dist"][0].tolist() == [0]


def test_capacity_retry_leaves_no_trace_of_the_first_attempt(ctx):
    """Two views of one table (sim3_table_ref.retry_scene): the crowded view's lists hold 70 > 64 candidates, so every view repeats at
    the longer capacity -- after the first attempt has accepted a match in the sparse view and marked its feature there
    (test_sim3_table_cpu.py holds the scene to that).  The sparse view's result is the one-view call's, byte for byte."""
    sc = Q.retry_scene()
    res, g, nm = _run(ctx, sc)
    one, _, _ = _run(ctx, Q.hand_scene(*Q.HAND_SHARED))
    for k in OUT:
        assert res[k][0].tobytes() == one[k][0].tobytes(), k
    assert res["matched_slot"][0].tobytes() == one["matched_slot"][0].tobytes() and res["n_matches"][0] == one["n_matches"][0] == 1
    assert res["best_idx"].tolist() == [[0, -1], [37, -1]] and nm.tolist() == [1, 1] and res["matched_slot"][1][37] == 0


def test_host_acceptance_stays_exact():
    """The host acceptance loops behind the device-made queries (what a handle too large for the acceptance kernel's LDS takes): a child
    process with CCM_WINDOW_HOST_ACCEPT=1 reruns the order cases, the capacity-retry scene (there: the lists grown on the host), the
    empty keyframe and the 257-point block edges."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CCM_WINDOW_HOST_ACCEPT="1", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k",
                          "hand_built or capacity_retry or empty_keyframe or (every_block_edge and 257)"], env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0 and " passed" in out.stdout, out.stdout[-2000:] + out.stderr[-1000:]


def test_sees_updates_queued_just_before(ctx, feat):
    sc = Q.loop_scene(feat, 400, 2)
    m = ORBmatcher(ctx=ctx)
    hs = _handles(ctx, sc)
    rng = np.random.default_rng(4)
    with _table(ctx, sc) as t:
        first = _call(m, t, hs, sc)
        g0, _ = _check(m, first, sc)
        other = dict(sc, slots=np.roll(sc["slots"], 7)[:300].copy())                # another list in between: the stamps of where[] tell them apart
        _check(m, _call(m, t, hs, other), other)
        back = _call(m, t, hs, sc)
        for k in OUT:
            assert first[k].tobytes() == back[k].tobytes(), k
        s = np.flatnonzero(g0["gate"][0] == Q.LG_SEARCHED)
        assert len(s) >= 30
        ids = sc["kfs"][0]["mp_id"].copy()
        ids[40:50] = sc["slots"][s[:10]]                                            # ten searched points are now observed
        sc["kfs"][0]["mp_id"] = ids
        moved = sc["slots"][s[10:20]]
        sc["rows"]["pos"][moved] += rng.normal(0, 0.02, (10, 3)).astype("f4")
        sc["rows"]["flags"][sc["slots"][s[20:30]]] |= R.BAD
        hs[0].map_points = ids                                                      # no synchronisation between these and the call
        t.update(moved, pos=sc["rows"]["pos"][moved])
        t.update(sc["slots"][s[20:30]], flags=sc["rows"]["flags"][sc["slots"][s[20:30]]])
        res = _call(m, t, hs, sc)
        g1, _ = _check(m, res, sc)
        assert (res["observed"][0][s[:10]] == 1).all() and (g1["gate"][:, s[20:30]] == Q.LG_SKIPPED).all()
    for h in hs:
        h.close()


# ---------------------------------------------------------------------------------------------------------------- misuse
def _raw(ctx, table, handles, slots, n_feat, n_levels=Q.N_LEVELS, drop=(), only_u=False):
    """The C call with sentinel-filled outputs.  Returns (rc, outputs untouched)."""
    lib = _lib.load()
    K = len(handles)
    slots = np.ascontiguousarray(slots, "i4")
    views = (_lib.LoopView * K)()
    ms = np.full(max(n_feat, 1), -1, "i4")
    for k, h in enumerate(handles):
        V = views[k].view
        V.kf = h
        V.Tcw[:] = [float(x) for x in R.CAMERAS[0][0].reshape(-1)]; V.Ow[:] = [float(x) for x in R.CAMERAS[0][1]]
        V.fx, V.fy, V.cx, V.cy = R.INTR
        V.min_x, V.max_x, V.min_y, V.max_y = R.BOUNDS
        views[k].matched_slot = None if "matched_slot_in" in drop else _lib.ptr(ms)
    prob = _lib.LoopProjectionProblem(K, None if "views" in drop else views, len(slots), None if "slot" in drop else _lib.ptr(slots), float(Q.LOG_SF),
                                      n_levels, None if "sf" in drop else _lib.ptr(Q.SCALE), TH)
    m = max(K * len(slots), 1)
    out = dict(best_idx=np.full(m, 12345, "i4"), observed=np.full(m, 99, np.uint8), matched_slot=np.full(K * max(n_feat, 1), 12345, "i4"),
               n_matches=np.full(K, 12345, "i4"), gate=np.full(m, 99, np.uint8), u=np.full(m, 7.5, "f4"), v=np.full(m, 7.5, "f4"),
               level=np.full(m, 12345, "i4"), best_dist=np.full(m, 12345, "i4"))
    g = lambda k: None if k in drop or (only_u and k in ("v", "level")) else _lib.ptr(out[k])  # noqa: E731
    res = _lib.LoopProjectionResult(*[g(k) for k in ("best_idx", "observed", "matched_slot", "n_matches", "gate", "u", "v", "level", "best_dist")])
    rc = lib.ccm_search_by_projection_table_frames(ctx.handle, C.c_void_p(table), C.byref(prob), C.byref(res))
    untouched = all((out[k] == (99 if k in ("gate", "observed") else 7.5 if k in "uv" else 12345)).all() for k in out)
    return rc, untouched


def test_misuse_returns_error_codes_and_leaves_the_outputs(ctx, feat):
    sc = Q.loop_scene(feat, 65, 2)
    hs = _handles(ctx, sc)
    other = _lib.Context(0)
    try:
        with _table(ctx, sc) as t:
            h = [x.handle for x in hs]
            rc, untouched = _raw(ctx, t.handle, h, sc["slots"], 64)
            assert rc >= 0 and not untouched                                         # the well-formed call runs
            for bad in ([3, 4, 3], [0, sc["capacity"]], [-1, 2]):                    # listed twice; outside the table
                assert _raw(ctx, t.handle, h, bad, 64) == (E_ARG, True), bad
            for drop in (("views",), ("slot",), ("sf",), ("best_idx",), ("observed",), ("matched_slot",), ("n_matches",), ("matched_slot_in",)):
                assert _raw(ctx, t.handle, h, sc["slots"], 64, drop=drop) == (E_ARG, True), drop
            assert _raw(ctx, t.handle, h, sc["slots"], 64, only_u=True) == (E_ARG, True)
            assert _raw(ctx, t.handle, h, sc["slots"], 64, n_levels=0) == (E_ARG, True)
            assert _raw(ctx, t.handle, h, sc["slots"], 64, n_levels=17) == (E_ARG, True)
            assert _raw(ctx, t.handle, [h[0], None], sc["slots"], 64) == (E_ARG, True)
            assert _raw(ctx, t.handle, [], sc["slots"], 64, drop=("views",)) == (0, True)       # zero keyframes: CCM_OK, nothing written
            with DeviceFrame(_view(sc["kfs"][0]), None, ctx=other) as fo, MapPointTable(sc["capacity"], ctx=other) as to:
                assert _raw(ctx, t.handle, [h[0], fo.handle], sc["slots"], 64) == (E_ARG, True)
                assert _raw(ctx, to.handle, h, sc["slots"], 64) == (E_ARG, True)
                assert _raw(other, t.handle, [fo.handle], sc["slots"], 64) == (E_ARG, True)
            m = ORBmatcher(ctx=ctx)
            _check(m, _call(m, t, hs, sc), sc)                                       # and the context still works
        orphan_t = MapPointTable(10, ctx=other)
        orphan_f = DeviceFrame(_view(sc["kfs"][0]), None, ctx=other)
    finally:
        other.close()
    with _table(ctx, sc) as t:
        assert _raw(ctx, orphan_t.handle, [hs[0].handle], [1, 2], 64) == (E_STATE, True)
        assert _raw(ctx, t.handle, [hs[0].handle, orphan_f.handle], sc["slots"], 64) == (E_STATE, True)
    orphan_t.close(); orphan_f.close()
    for x in hs:
        x.close()
