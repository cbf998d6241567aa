"""The device-resident map-point table (include/ccm_hot.h "map-point table") on the GPU: the table against a numpy model,
ccm_frame_search_local_points against the numpy restatement tests/search_local_points_ref.py (frustum bit for bit, every wave and
workgroup boundary of the order-preserving compaction), its matches against the handle matcher and the CPU oracle fed the
restatement's arrays, the first loop and the seen stamps, the pose from the table against the host-buffer pose, misuse and churn."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import optimizer_cases as C_
import search_local_points_ref as R
from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher
from motioncheck_ccm_slam_amd.optimizer import Optimizer
from motioncheck_ccm_slam_amd.orb import ORBextractor
from motioncheck_ccm_slam_amd.tracking import MapPointTable, Tracking

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -7
COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")
CAM = R.camera()


def _bits(a):
    return np.ascontiguousarray(a, "f4").view("u4")


def _slp(frame, table, cam=CAM, sf=R.SCALE, th=1.0):
    return Tracking.SearchLocalPoints(frame, table, cam[0], R.INTR, sf, Ow=cam[1], th=th, log_scale_factor=R.LOG_SF, taps=True)


def _small_frame(ctx, n=40, seed=3):
    rng = np.random.default_rng(seed)
    fr = FrameGridView(rng.uniform(0, 752, n), rng.uniform(0, 480, n), rng.integers(0, 8, n), rng.integers(0, 256, (n, 32)))
    return DeviceFrame(fr, None, ctx=ctx)


def _check_frustum(res, ref):
    """in_view_slot, proj_x / y and view_cos bit for bit; level equal except on ambiguous points (within 1 there)."""
    assert res["n_to_match"] == len(ref["in_view_slot"]) and (res["in_view_slot"] == ref["in_view_slot"]).all()
    for k in ("proj_x", "proj_y", "view_cos"):
        assert (_bits(res[k]) == _bits(ref[k])).all(), k
    d = res["level"] - ref["level"]
    amb = ref["ambiguous"]
    assert (d[~amb] == 0).all() and (np.abs(d[amb]) <= 1).all()
    return int(amb.sum())


@pytest.fixture(scope="module")
def scene(ctx):
    """20,000 random points in a table, loaded once and left unchanged."""
    rows = R.random_points(20000, 1)
    t = MapPointTable(20000, ctx=ctx)
    t.update(np.arange(20000), **{k: rows[k] for k in COLS})
    yield rows, t
    t.close()


# ---------------------------------------------------------------------------------------------------------------- 1. table
@pytest.mark.parametrize("cap", [1, 63, 64, 65, 1000])
def test_table_updates_match_a_numpy_model(ctx, cap):
    rng = np.random.default_rng(cap)
    model = dict(pos=np.zeros((cap, 3), "f4"), normal=np.zeros((cap, 3), "f4"), min_dist=np.zeros(cap, "f4"), max_dist=np.zeros(cap, "f4"),
                 desc=np.zeros((cap, 32), np.uint8), flags=np.zeros(cap, np.uint8))

    def rows(n):
        return dict(pos=rng.normal(0, 5, (n, 3)).astype("f4"), normal=rng.normal(0, 1, (n, 3)).astype("f4"), min_dist=rng.uniform(0, 1, n).astype("f4"),
                    max_dist=rng.uniform(1, 9, n).astype("f4"), desc=rng.integers(0, 256, (n, 32), dtype=np.uint8),
                    flags=rng.integers(0, 8, n).astype(np.uint8))

    def same(t):
        got = t.fetch(np.arange(cap))
        return all((got[k] == model[k]).all() for k in COLS) and (got["seen"] == 0).all()
    with MapPointTable(cap, ctx=ctx) as t:
        assert t.capacity == cap and same(t)                      # a fresh table holds zeros
        s = rng.permutation(cap)[:max(1, cap // 2)]               # scattered slots, every column
        r = rows(len(s)); t.update(s, **r)
        for k in COLS:
            model[k][s] = r[k]
        assert same(t)
        s = rng.permutation(cap)[:max(1, cap // 3)]               # column-wise: positions only (BA), then flags only (culling)
        r = rows(len(s)); t.update(s, pos=r["pos"]); model["pos"][s] = r["pos"]
        t.update(s, flags=r["flags"]); model["flags"][s] = r["flags"]
        assert same(t)
        for _ in range(3):                                        # one slot again and again, and twice within one update: the last row wins
            s = np.array([cap - 1, 0, cap - 1], "i4")
            r = rows(3); t.update(s, **r)
            for k in COLS:
                model[k][s[1:]] = r[k][1:]
        assert same(t)
        t.update(np.zeros(0, "i4"))                               # n = 0
        assert same(t)
        for bad in (cap, -1):                                     # a slot outside the table: CCM_E_ARG, nothing written
            s = np.array([0, bad], "i4"); r = rows(2)
            with pytest.raises(_lib.CcmError) as e:
                t.update(s, **r)
            assert e.value.code == E_ARG
            with pytest.raises(_lib.CcmError) as e:
                t.fetch(s)
            assert e.value.code == E_ARG
        assert same(t)
        for bad in ([0, 0], [cap], [-1]):                         # order: a duplicate or a slot outside the table
            with pytest.raises(_lib.CcmError) as e:
                t.set_order(bad)
            assert e.value.code == E_ARG


# ---------------------------------------------------------------------------------------------------------------- 2. frustum
@pytest.mark.parametrize("n_order", [1, 63, 64, 65, 1023, 1024, 1025, 20000])
def test_frustum_bit_exact_at_every_compaction_boundary(ctx, scene, n_order):
    rows, t = scene
    order = np.arange(20000 - n_order, 20000)                     # a list that does not start at slot 0
    t.set_order(order)
    ref = R.replay([], rows, order, *CAM)
    with _small_frame(ctx) as f:
        n_amb = _check_frustum(_slp(f, t), ref)
    print("order %d: %d in view, %d ambiguous levels" % (n_order, len(ref["in_view_slot"]), n_amb))
    if n_order == 20000:
        assert len(ref["in_view_slot"]) >= 1000 and n_amb <= 0.001 * len(ref["in_view_slot"])
        assert (np.bincount(ref["gate"], minlength=6)[1:] >= 50).all() and (np.bincount(ref["level"], minlength=8) > 0).all()


def test_frustum_orders_and_extremes(ctx, scene):
    rows, t = scene
    rng = np.random.default_rng(8)
    with _small_frame(ctx) as f, DeviceFrame(FrameGridView(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 32))), None, ctx=ctx) as empty:
        t.set_order(None)                                         # ascending slot over the LIVE slots
        full = R.replay([], rows, None, *CAM)
        _check_frustum(_slp(f, t), full)
        r0 = _slp(empty, t)                                       # an empty frame: the frustum still runs, no matcher
        _check_frustum(r0, full)
        assert r0["nmatches"] == 0 and len(r0["match"]) == 0
        perm = rng.permutation(20000)[:5000]                      # permuted, and shorter than the live set
        t.set_order(perm)
        ref = R.replay([], rows, perm, *CAM)
        _check_frustum(_slp(f, t), ref)
        assert 1000 < len(ref["in_view_slot"]) < len(full["in_view_slot"])
        t.set_order(np.zeros(0, "i4"))                            # an empty order
        res = _slp(f, t)
        assert res["n_to_match"] == 0 and res["nmatches"] == 0 and (res["match"] == -1).all()
        t.set_order(None)
        away = R.camera(t=(0.0, 0.0, -100.0))                     # every point behind the camera: none in view
        assert len(R.replay([], rows, None, *away)["in_view_slot"]) == 0
        res = _slp(f, t, cam=away)
        assert res["n_to_match"] == 0 and res["nmatches"] == 0 and (res["mp_id"] == -1).all()
        iv = full["in_view_slot"]                                 # all in view: a table of the visible points only
        with MapPointTable(len(iv), ctx=ctx) as t2:
            sub = {k: rows[k][iv] for k in COLS}
            t2.update(np.arange(len(iv)), **sub)
            ref = R.replay([], sub, None, *CAM)
            assert len(ref["in_view_slot"]) == len(iv)
            _check_frustum(_slp(f, t2), ref)


def test_frustum_edge_rows(ctx):
    """A point on the camera plane, u == max_x exactly, and the level boundaries of PredictScale (identity camera)."""
    rows = R.edge_points()
    n = len(rows["flags"])
    with MapPointTable(n, ctx=ctx) as t, _small_frame(ctx) as f:
        t.update(np.arange(n), **rows)
        ref = R.replay([], rows, None, *R.IDENTITY)
        res = _slp(f, t, cam=R.IDENTITY)
        n_amb = _check_frustum(res, ref)
        print("edge rows: %d ambiguous levels of %d" % (n_amb, n))
        assert (ref["in_view_slot"] == np.arange(1, n)).all() and res["proj_x"][0] == np.float32(752)
        assert (ref["level"][1:].reshape(8, 8)[:, 0] == np.arange(8)).all()


# ---------------------------------------------------------------------------------------------------------------- 3. matching
@pytest.fixture(scope="module")
def matchable(ctx):
    """One extracted frame, its features as map points behind the inverse pose, 3,000 random points, in a permuted slot order."""
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    kps, desc = ex(synth.frame(1))
    sf, is2 = ex.GetScaleFactors(), ex.GetInverseScaleSigmaSquares()
    fr = FrameGridView(kps["x"], kps["y"], kps["octave"], desc)
    n = len(kps)
    rows = R.concat(R.matchable_points(fr.kx, fr.ky, fr.oct, desc, *CAM, seed=4), R.random_points(3000, 2))
    rng = np.random.default_rng(6)
    slot_of = rng.permutation(n + 3000).astype("i4")              # row r lives in slot slot_of[r]
    table_rows = {k: np.empty_like(rows[k]) for k in COLS}
    for k in COLS:
        table_rows[k][slot_of] = rows[k]
    ids = np.where(rng.random(n) < 0.1, slot_of[:n], -1).astype("i4")     # a tenth of the features already hold their point
    return dict(fr=fr, angle=kps["angle"], sf=sf, is2=is2, rows=table_rows, ids=ids, n=n, slot_of=slot_of)


def _matching(ctx, oracle, S, th):
    fr, rows, ids = S["fr"], S["rows"], S["ids"]
    cap = len(rows["flags"])
    ref = R.replay(ids, rows, None, *CAM)
    assert ref["ambiguous"].sum() == 0                            # else the restatement's levels are not the only valid ones
    nq = len(ref["in_view_slot"])
    iv = np.ones(nq, bool)
    m = ORBmatcher(0.8, ctx=ctx)
    with MapPointTable(cap, ctx=ctx) as t, DeviceFrame(fr, S["angle"], ctx=ctx) as h, DeviceFrame(fr, S["angle"], ctx=ctx) as h2:
        t.update(np.arange(cap), **rows)
        h.map_points = ids
        res = _slp(h, t, sf=S["sf"], th=th)
        _check_frustum(res, ref)
        h2.map_points = ref["ids"]
        hn, hmatch, hocc = m.SearchByProjectionHandle(h2, S["sf"], iv, ref["level"], ref["view_cos"], ref["proj_x"], ref["proj_y"], ref["desc"],
                                                      ref["has_obs"], ref["occupied"], th, query_mp_id=ref["in_view_slot"])
        on, omatch, oocc = oracle.search_by_projection(fr.kx, fr.ky, fr.oct, fr.desc, fr.min_x, fr.min_y, fr.inv_w, fr.inv_h, S["sf"], iv,
                                                       ref["level"], ref["view_cos"], ref["proj_x"], ref["proj_y"], ref["desc"], ref["has_obs"],
                                                       ref["occupied"], th, 0.8)
        assert hn == on and (hmatch == omatch).all() and (hocc == oocc).all()
        want = np.where(omatch >= 0, ref["in_view_slot"][np.maximum(omatch, 0)], -1)
        print("th %g: %d in view, %d matches" % (th, nq, on))
        assert res["nmatches"] == on and (res["match"] == want).all() and (res["occupied"] == oocc).all()
        assert (res["mp_id"] == h2.map_points).all() and (h.map_points == res["mp_id"]).all()
        assert (res["mp_id"] == np.where(want >= 0, want, ref["ids"])).all()
        assert on >= 300
    return res


@pytest.mark.parametrize("th", [1.0, 5.0])
def test_matching_equals_handle_matcher_and_oracle(ctx, oracle, matchable, th):
    _matching(ctx, oracle, matchable, th)


def test_matching_with_host_acceptance():
    """The host acceptance loops behind the device-made queries: a child process with CCM_WINDOW_HOST_ACCEPT=1 reruns the matching tests."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CCM_WINDOW_HOST_ACCEPT="1", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", "matching_equals"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-1000:]


# ---------------------------------------------------------------------------------------------------------------- 4. first loop, stamps
def test_first_loop_and_stamps(ctx, scene):
    rows, t0 = scene
    rows = {k: v[:3000].copy() for k, v in rows.items()}
    rng = np.random.default_rng(12)
    rows["flags"][rng.permutation(3000)[:300]] |= R.BAD           # bad points, with and without observations
    full = R.replay([], rows, None, *CAM)
    vis = full["in_view_slot"]
    bad = np.flatnonzero(rows["flags"] & R.BAD)
    nobs = vis[(rows["flags"][vis] & R.HAS_OBS) == 0]
    assert len(vis) > 500 and len(nobs) > 10

    def frame_ids(seed, n=40):
        g = np.random.default_rng(seed)
        ids = np.full(n, -1, "i4")
        ids[0:8] = g.choice(bad, 8, replace=False)                # bad: cleared
        ids[8:20] = g.choice(vis, 12, replace=False)              # good and visible: seen, not projected again
        ids[20:24] = g.choice(nobs, 4, replace=False)             # without observations: occupied stays 0
        ids[24:26] = ids[8]                                       # one slot held by several features
        return ids
    with MapPointTable(3000, ctx=ctx) as t, _small_frame(ctx, seed=1) as fa, _small_frame(ctx, seed=2) as fb:
        t.update(np.arange(3000), **rows)
        got = []
        for f, seed in ((fa, 1), (fb, 2)):                        # two calls in a row on one table
            ids = frame_ids(seed)
            f.map_points = ids
            ref = R.replay(ids, rows, None, *CAM)
            res = _slp(f, t)
            _check_frustum(res, ref)
            assert (ref["ids"][:8] == -1).all() and (ref["ids"][8:26] == ids[8:26]).all() and not np.isin(ids[8:26], ref["in_view_slot"]).any()
            assert (ref["occupied"][20:24] == 0).all() and ref["occupied"][8:20].any()
            new = res["match"] >= 0
            assert (res["mp_id"][~new] == ref["ids"][~new]).all() and (res["occupied"][~new] == ref["occupied"][~new]).all()
            assert (res["mp_id"][new] == res["match"][new]).all() and (f.map_points == res["mp_id"]).all()
            got.append(res)
        stamps = t.fetch(np.arange(3000))["seen"]
        assert set(np.unique(stamps)) == {0, 1, 2}                # the stamps are the call counter
        for (f, seed), first in zip(((fa, 1), (fb, 2)), got):     # each call equals the same call on a fresh table
            with MapPointTable(3000, ctx=ctx) as fresh:
                fresh.update(np.arange(3000), **rows)
                f.map_points = frame_ids(seed)
                res = _slp(f, fresh)
                for k in ("in_view_slot", "match", "mp_id", "occupied", "level"):
                    assert (res[k] == first[k]).all(), k
                assert res["nmatches"] == first["nmatches"]


# ---------------------------------------------------------------------------------------------------------------- 5. pose
def _pose7(Tcw):
    T16 = np.concatenate([np.asarray(Tcw, "f4").reshape(3, 4), np.array([[0, 0, 0, 1]], "f4")]).copy()
    p7 = np.zeros(7)
    assert _lib.load().ccm_pose_from_mat4f(_lib.ptr(T16), _lib.ptr(p7)) == 0
    return p7


def test_pose_from_table_and_track_local_map(ctx, matchable):
    S = matchable
    fr, rows, n = S["fr"], S["rows"], S["n"]
    cap = len(rows["flags"])
    intr = np.array(R.INTR, "f8")
    rng = np.random.default_rng(2)
    ids = np.where(rng.random(n) < 0.6, S["slot_of"][:n], -1).astype("i4")
    wrong = np.flatnonzero(ids >= 0)[::11]
    ids[wrong] = S["slot_of"][rng.integers(0, n, len(wrong))]     # some wrong correspondences: outliers
    xyz = rows["pos"].astype("f8")
    pose = _pose7(CAM[0])
    pose[4:] += [0.02, -0.01, 0.03]
    with MapPointTable(cap, ctx=ctx) as t, DeviceFrame(fr, S["angle"], ctx=ctx) as h:
        t.update(np.arange(cap), **rows)
        h.map_points = ids
        a = Optimizer.PoseOptimizationFrame(h, pose, intr, xyz, S["is2"])
        b = Tracking.PoseOptimizationTable(h, t, pose, intr, S["is2"])
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]             # bit for bit
        assert a[2] > 300 and a[1].sum() >= len(wrong) // 2 and (a[0] != pose).any()
        # a slot that is not LIVE: CCM_E_ARG
        slot = int(ids[ids >= 0][3])
        t.update([slot], flags=[0])
        with pytest.raises(_lib.CcmError) as e:
            Tracking.PoseOptimizationTable(h, t, pose, intr, S["is2"])
        assert e.value.code == E_ARG
        t.update(np.arange(cap), flags=rows["flags"])
        # TrackLocalMap through the mirror against the host-buffer chain fed the restatement's arrays
        start = np.where(rng.random(n) < 0.2, S["slot_of"][:n], -1).astype("i4")
        h.map_points = start
        s, p7, outl, inl = Tracking.TrackLocalMap(h, t, pose, CAM[0], R.INTR, S["sf"], S["is2"], Ow=CAM[1], log_scale_factor=R.LOG_SF)
        ref = R.replay(start, rows, None, *CAM)
        with DeviceFrame(fr, S["angle"], ctx=ctx) as h2:
            h2.map_points = ref["ids"]
            hn, hmatch, _ = ORBmatcher(0.8, ctx=ctx).SearchByProjectionHandle(
                h2, S["sf"], np.ones(len(ref["level"]), bool), ref["level"], ref["view_cos"], ref["proj_x"], ref["proj_y"], ref["desc"],
                ref["has_obs"], ref["occupied"], 1.0, query_mp_id=ref["in_view_slot"])
            rp, ro, _ = Optimizer.PoseOptimizationFrame(h2, pose, intr, xyz, S["is2"])
            assert s["nmatches"] == hn and (s["mp_id"] == h2.map_points).all()
            assert (p7 == rp).all() and (outl == ro).all() and inl == int(((h2.map_points >= 0) & (ro == 0)).sum()) and inl > 300


def test_pose_from_table_at_the_compaction_edges(ctx):
    """k_frame_pose_gather on a table across a 1024-block with every second 64-group empty (1025 features): the table form equals the array call
    on the gathered problem bit for bit; the points are the table's float32 positions."""
    N = 1025
    fc = C_.frame_case(N, "alternate")
    has = fc["mask"]
    is2 = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx).GetInverseScaleSigmaSquares()
    rows = R.random_points(N, 5)
    rows["pos"] = fc["table"].astype("f4")
    assert (rows["pos"].astype("f8") == fc["table"]).all()           # positions already went through float32
    pts, obs, info = C_.gathered(fc, is2)
    rp, ro, rn = Optimizer.PoseOptimizationClient(fc["pose"][None], fc["intr"][None], np.array([0, has.sum()], "i4"), pts, obs, info, ctx=ctx)
    desc = np.random.default_rng(N).integers(0, 256, (N, 32), dtype=np.uint8)
    with MapPointTable(N, ctx=ctx) as t, DeviceFrame(FrameGridView(fc["kx"], fc["ky"], fc["oct"], desc, *C_.FRAME_BOUNDS), None, ctx=ctx) as h:
        t.update(np.arange(N), **{k: rows[k] for k in COLS})
        h.map_points = fc["ids"]
        p7, outl, ni = Tracking.PoseOptimizationTable(h, t, fc["pose"], fc["intr"], is2)
    assert (p7 == rp[0]).all() and ni == rn[0] and (outl[has] == ro).all() and (outl[~has] == 0).all()
    assert has.sum() == 512 and ni > 400 and ro.sum() >= 60


# ---------------------------------------------------------------------------------------------------------------- 6. misuse, churn
def test_misuse_returns_error_codes(ctx, scene):
    rows, t = scene
    lib = _lib.load()
    other = _lib.Context(0)
    try:
        with _small_frame(ctx) as f:
            with _small_frame(other) as fo:                       # a table of context A with context B (and B's own frame)
                with pytest.raises(_lib.CcmError) as e:
                    Tracking.SearchLocalPoints(fo, t, CAM[0], R.INTR, R.SCALE, Ow=CAM[1])
                assert e.value.code == E_ARG
            u = _lib.MapUpdate(0, None, None, None, None, None, None, None)
            assert lib.ccm_map_table_update(other.handle, C.c_void_p(t.handle), C.byref(u)) == E_ARG
            # an id of a slot that is not LIVE, and one outside the table: CCM_E_ARG, the frame's ids as they were
            with MapPointTable(100, ctx=ctx) as small:
                small.update(np.arange(50), **{k: rows[k][:50] for k in COLS})
                for bad in (70, 100, 1 << 30):
                    ids = np.full(f.n, -1, "i4"); ids[:3] = [4, bad, 7]
                    f.map_points = ids
                    with pytest.raises(_lib.CcmError) as e:
                        _slp(f, small)
                    assert e.value.code == E_ARG and (f.map_points == ids).all()
                    with pytest.raises(_lib.CcmError) as e:
                        Tracking.PoseOptimizationTable(f, small, np.array([0, 0, 0, 1, 0, 0, 0.0]), np.array(R.INTR), R.SCALE)
                    assert e.value.code == E_ARG
                with pytest.raises(_lib.CcmError) as e:           # more levels than CCM_MAX_LEVELS
                    _slp(f, small, sf=np.ones(17, "f4"))
                assert e.value.code == E_ARG
        orphan = MapPointTable(10, ctx=other)
    finally:
        other.close()
    # the context is gone: only capacity and destroy
    assert lib.ccm_map_table_capacity(C.c_void_p(orphan.handle)) == 10
    u = _lib.MapUpdate(0, None, None, None, None, None, None, None)
    assert lib.ccm_map_table_update(ctx.handle, C.c_void_p(orphan.handle), C.byref(u)) == E_STATE
    assert lib.ccm_map_table_set_order(ctx.handle, C.c_void_p(orphan.handle), 0, None) == E_STATE
    assert lib.ccm_map_table_fetch(ctx.handle, C.c_void_p(orphan.handle), 0, *([None] * 8)) == E_STATE
    with _small_frame(ctx) as f:                                  # a live frame with the orphaned table
        with pytest.raises(_lib.CcmError) as e:
            _slp(f, orphan)
        assert e.value.code == E_STATE
        with pytest.raises(_lib.CcmError) as e:
            Tracking.PoseOptimizationTable(f, orphan, np.array([0, 0, 0, 1, 0, 0, 0.0]), np.array(R.INTR), R.SCALE)
        assert e.value.code == E_STATE
    orphan.close()


def test_churn_then_still_exact(ctx, scene):
    rows, t = scene
    rng = np.random.default_rng(31)
    live = []
    for i in range(200):
        cap = int(rng.integers(1, 3000))
        tb = MapPointTable(cap, ctx=ctx)
        s = rng.integers(0, cap, min(cap, 64))
        tb.update(s, pos=rows["pos"][:len(s)], flags=rows["flags"][:len(s)])
        live.append(tb)
        if len(live) > 3 or rng.random() < 0.5:                   # a few alive at a time, destroyed out of order
            live.pop(int(rng.integers(0, len(live)))).close()
    for tb in live:
        tb.close()
    t.set_order(None)
    with _small_frame(ctx) as f:
        _check_frustum(_slp(f, t), R.replay([], rows, None, *CAM))
