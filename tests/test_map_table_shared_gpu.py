"""Table views on the GPU (ccm_map_table_attach, include/ccm_hot.h "map-point table"): one table's rows named by handles of two
contexts.  Every comparison is bit for bit: the same kernels produce both sides -- a call through a view against the same call made
entirely inside one context, which the other test files hold to their references.  Equivalence of every entry point that takes a
table, visibility of writes that return without synchronising, scratch per handle, lifetime, and two contexts used from two threads
at once."""
import ctypes as C
import threading

import numpy as np
import pytest

import fuse_table_ref as R
import map_refresh_ref as MR
import search_local_points_ref as S
import sim3_table_ref as Q
import track_motion_model_ref as M
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher
from motioncheck_ccm_slam_amd.tracking import MapPointTable, Tracking

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -7
COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")
K4 = np.array(MR.INTR, "f4")
JOIN_S = 120.0                                    # a thread that has not finished by then fails the test


def _same(a, b):
    """Byte-equal, through dicts, lists, tuples, MotionModelResults, arrays and scalars."""
    if hasattr(a, "__dict__") and not isinstance(a, np.ndarray):
        a, b = a.__dict__, b.__dict__
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _view(kf):
    return FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"].reshape(-1, 32))


def _frame(ctx, kf, ids=None):
    h = DeviceFrame(_view(kf), None, ctx=ctx)
    if ids is not None:
        h.map_points = ids
    return h


def _load(t, rows):
    live = np.flatnonzero(rows["flags"] & R.LIVE)                 # the rows that are not LIVE are never written: a fresh table holds zeros
    t.update(live, **{k: rows[k][live] for k in COLS})
    return t


def _all_rows(t):
    got = t.fetch(np.arange(t.capacity))
    return {k: got[k] for k in COLS}


@pytest.fixture(scope="module")
def ctx_b():
    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------------------ the scenes
@pytest.fixture(scope="module")
def world():
    """One table for Fuse, the two ComputeSim3 matchers, SearchLocalPoints and the pose: a SearchByProjection(Scw) scene (a Fuse scene
    with vpMatched) of 65 points and 3 keyframes in the slots [0, c1), a SearchBySim3 scene of two 65 x 65 pairs behind it.  65 crosses
    the wave boundary of every compaction.  Built once and left unchanged."""
    feat = R.synthetic_features(600, 7)
    loop = Q.loop_scene(feat, 65, 3)
    sim3 = Q.sim3_scene(feat, 65, 65, 2)
    c1, c2 = loop["capacity"], sim3["capacity"]
    rows = {k: np.concatenate([loop["rows"][k], sim3["rows"][k]]) for k in COLS}
    for kf in sim3["kfs"]:
        ids = kf["mp_id"]
        kf["mp_id"] = np.where((ids >= 0) & (ids < c2), ids + c1, ids).astype("i4")
    live = np.flatnonzero((loop["rows"]["flags"] & (R.LIVE | R.BAD)) == R.LIVE)
    track_ids = np.full(64, -1, "i4"); track_ids[:6] = live[:6]   # the tracked frame: keyframe 0's features, six of them holding points
    return dict(rows=rows, capacity=c1 + c2, loop=loop, sim3=sim3, track_ids=track_ids, order=live.astype("i4"))


class Handles:
    """The world's keyframes and the tracked frame as handles of one context."""

    def __init__(self, ctx, w):
        self.ctx = ctx
        self.m = ORBmatcher(ctx=ctx)
        self.loop = [_frame(ctx, kf, kf["mp_id"]) for kf in w["loop"]["kfs"]]
        self.sim3 = {id(kf): _frame(ctx, kf, kf["mp_id"]) for kf in w["sim3"]["kfs"]}
        self.track = _frame(ctx, w["loop"]["kfs"][0])

    def close(self):
        for h in self.loop + list(self.sim3.values()) + [self.track]:
            h.close()


def _fuse(H, t, w, par):
    sc = w["loop"]; kfs = sc["kfs"]
    return H.m.FuseSelectTableFrames(t, H.loop, [k["Tcw"] for k in kfs], [k["Ow"] for k in kfs], R.INTR, R.BOUNDS, sc["slots"], R.SCALE, R.INV_SIGMA2,
                                     log_scale_factor=R.LOG_SF, taps=True, **par)


def _loop(H, t, w):
    sc = w["loop"]; kfs = sc["kfs"]
    return H.m.SearchByProjectionTableFrames(t, H.loop, [k["Tcw"] for k in kfs], [k["Ow"] for k in kfs], R.INTR, R.BOUNDS, sc["slots"],
                                             [k["matched_slot"] for k in kfs], Q.SCALE, th=10.0, log_scale_factor=Q.LOG_SF, taps=True)


def _sim3(H, t, w):
    return H.m.SearchBySim3TableFrames(t, [dict(p, kf1=H.sim3[id(p["kf1"])], kf2=H.sim3[id(p["kf2"])]) for p in w["sim3"]["pairs"]], Q.SCALE, th=7.5,
                                       log_scale_factor1=Q.LOG_SF, taps=True)


def _slp(H, t, w):
    kf = w["loop"]["kfs"][0]
    H.track.map_points = w["track_ids"]
    return Tracking.SearchLocalPoints(H.track, t, kf["Tcw"], R.INTR, R.SCALE, Ow=kf["Ow"], th=3.0, log_scale_factor=R.LOG_SF, taps=True, ctx=H.ctx)


def _pose7(Tcw):
    T16 = np.concatenate([np.asarray(Tcw, "f4").reshape(3, 4), np.array([[0, 0, 0, 1]], "f4")]).copy()
    p7 = np.zeros(7)
    assert _lib.load().ccm_pose_from_mat4f(_lib.ptr(T16), _lib.ptr(p7)) == 0
    return p7


def _pose(H, t, w):
    """The pose from the table on the ids SearchLocalPoints left in the tracked frame."""
    return Tracking.PoseOptimizationTable(H.track, t, _pose7(w["loop"]["kfs"][0]["Tcw"]), np.array(R.INTR, "f8"), R.INV_SIGMA2, ctx=H.ctx)


@pytest.fixture(scope="module")
def handles_b(ctx_b, world):
    H = Handles(ctx_b, world)
    yield H
    H.close()


@pytest.fixture(scope="module")
def alone(ctx_b, world, handles_b):
    """Every call of the world made entirely inside context B on a table of its own: the existing path.  Computed once."""
    H, w = handles_b, world
    with _load(MapPointTable(w["capacity"], ctx=ctx_b), w["rows"]) as t:
        out = dict(fuse=[_fuse(H, t, w, par) for par in R.PARAMS], sim3=_sim3(H, t, w), loop=_loop(H, t, w), slp=_slp(H, t, w), pose=_pose(H, t, w),
                   rows=_all_rows(t))
    assert all(f["n_searched"] >= 10 for f in out["fuse"]) and out["sim3"]["total"] >= 10 and out["loop"]["total"] >= 3
    assert out["slp"]["n_to_match"] >= 20 and out["slp"]["nmatches"] >= 5
    return out


@pytest.fixture(scope="module")
def refresh_world(ctx_b):
    """tests/map_refresh_ref.py's scene (every observation count, ties, a point on a camera centre) with its keyframe handles in B."""
    sc = MR.scene(1)
    rows = MR.table_rows(2)
    rows["pos"][sc["slot"]] = sc["pos"]
    kfs = []
    for kf in sc["kfs"]:
        h = _frame(ctx_b, kf, np.full(len(kf["kx"]), -1, "i4"))
        h.set_camera(K4, kf["sf"], kf["sigma2"]); h.set_pose(kf["Tcw"], kf["Ow"])
        kfs.append(h)
    yield sc, rows, kfs
    for h in kfs:
        h.close()


def _refresh(t, sc, kfs, **kw):
    return t.refresh(sc["slot"], kfs, sc["obs_first"], sc["obs_kf"], sc["obs_feat"], sc["ref_kf"], sc["ref_feat"], **kw)


# ---------------------------------------------------------------------------------------------------------------- 1. equivalence
def test_calls_through_a_view_equal_the_calls_inside_one_context(ctx, ctx_b, world, handles_b, alone):
    H, w = handles_b, world
    with _load(MapPointTable(w["capacity"], ctx=ctx), w["rows"]) as root, root.attach(ctx_b) as view:
        assert view.capacity == root.capacity == w["capacity"] and root.handles() == view.handles() == 2
        for par, want in zip(R.PARAMS, alone["fuse"]):
            assert _same(_fuse(H, view, w, par), want), par
        assert _same(_sim3(H, view, w), alone["sim3"])
        assert _same(_loop(H, view, w), alone["loop"])
        assert _same(_slp(H, view, w), alone["slp"])
        assert _same(_pose(H, view, w), alone["pose"])
        assert _same(_all_rows(view), alone["rows"]) and _same(_all_rows(root), alone["rows"])


@pytest.mark.parametrize("fetch", [True, False], ids=["result", "no_result"])
@pytest.mark.parametrize("what", [MR.DESCRIPTOR, MR.NORMAL_DEPTH, MR.DESCRIPTOR | MR.NORMAL_DEPTH], ids=["descriptor", "normal_depth", "both"])
def test_refresh_through_a_view_equals_refresh_inside_one_context(ctx, ctx_b, refresh_world, what, fetch):
    sc, rows, kfs = refresh_world
    full = np.arange(MR.CAPACITY)
    with MapPointTable(MR.CAPACITY, ctx=ctx_b) as solo:
        solo.update(full, **rows)
        want = _refresh(solo, sc, kfs, what=what, fetch=fetch)
        want_rows = _all_rows(solo)
    assert not _same(want_rows, {k: rows[k] for k in COLS})       # the call changed rows
    with MapPointTable(MR.CAPACITY, ctx=ctx) as root:
        root.update(full, **rows)
        with root.attach(ctx_b) as view:
            assert _same(_refresh(view, sc, kfs, what=what, fetch=fetch), want)
            assert _same(_all_rows(root), want_rows)              # through the other handle first: it must see the view's write
            assert _same(_all_rows(view), want_rows)


def _tmm_scene():
    """TrackWithMotionModel's situation without an extraction: 200 synthetic features as the last frame, one map point behind each plus 65
    random ones in permuted slots, the current frame = the same features moved by (-5, +3) pixels."""
    f = R.synthetic_features(200, 11)
    cam0 = S.camera()
    n = 200
    rows = S.concat(S.matchable_points(f["kx"], f["ky"], f["oct"], f["desc"], *cam0, seed=4), S.random_points(65, 5))
    rng = np.random.default_rng(6)
    slot_of = rng.permutation(n + 65).astype("i4")
    table = {k: np.empty_like(v) for k, v in rows.items()}
    for k in rows:
        table[k][slot_of] = rows[k]
    ids = np.where(rng.random(n) < 0.9, slot_of[:n], -1).astype("i4")
    cur = dict(f, kx=(f["kx"] - np.float32(5)).astype("f4"), ky=(f["ky"] + np.float32(3)).astype("f4"))
    return dict(last=f, cur=cur, rows=table, ids=ids, cam=M.shifted_camera(cam0[0], -5.0, 3.0))


def test_track_with_motion_model_through_a_view(ctx, ctx_b):
    T = _tmm_scene()
    cap = len(T["rows"]["flags"])

    def run(t):
        with _frame(ctx_b, T["last"], T["ids"]) as hl, _frame(ctx_b, T["cur"], np.arange(200, dtype="i4") % cap) as hc:
            start = _pose7(T["cam"]); start[4:] += [0.02, -0.01, 0.03]
            res = Tracking.TrackWithMotionModel(hc, hl, t, T["cam"], start, np.array(S.INTR, "f8"), S.SCALE, R.INV_SIGMA2, check_ori=False, taps=True, ctx=ctx_b)
            assert (hc.map_points == res.mp_id).all()
        return res
    with MapPointTable(cap, ctx=ctx_b) as solo:
        solo.update(np.arange(cap), **T["rows"])
        want = run(solo)
    assert want.posed and want.n_matches >= 50 and want.n_inliers >= 20
    with MapPointTable(cap, ctx=ctx) as root:
        root.update(np.arange(cap), **T["rows"])                  # returns with the scatter queued on A's stream
        with root.attach(ctx_b) as view:
            assert _same(run(view), want)
            assert _same(_all_rows(view), {k: T["rows"][k] for k in COLS})


# ---------------------------------------------------------------------------------------------------------------- 2. visibility
BIG = 1 << 17


def test_unsynchronised_updates_are_seen_through_the_other_handle(ctx, ctx_b):
    """A queues full-capacity updates that return with their copies and scatters still queued; B's view fetches at once and must see the
    last one.  A missing event wait can still pass by luck on a fast queue: the test cannot prove the wait, only catch its absence when
    the reader overtakes."""
    rows = S.random_points(BIG, 3)
    full = np.arange(BIG, dtype="i4")
    probe = np.concatenate([[0, BIG - 1], np.random.default_rng(1).permutation(BIG)[:1000]]).astype("i4")
    with MapPointTable(BIG, ctx=ctx) as root, root.attach(ctx_b) as view:
        for i in range(4):
            root.update(full, **dict(rows, pos=np.full((BIG, 3), float(i), "f4")))
        got = view.fetch(probe)
        assert (got["pos"] == 3.0).all()
        for k in COLS[1:]:
            assert _same(got[k], rows[k][probe]), k
        for i in range(4):                                        # and the other way round
            view.update(full, pos=np.full((BIG, 3), 10.0 + i, "f4"))
        assert (root.fetch(probe)["pos"] == 13.0).all()


def test_an_unsynchronised_refresh_is_seen_through_the_other_handle(ctx, ctx_b, refresh_world):
    """B queues full-capacity updates of the rows behind the refresh scene and then a refresh without a result; A fetches and runs
    SearchLocalPoints at once.  As above, a missing wait can still pass by luck on a fast queue."""
    sc, rows, kfs = refresh_world
    far = S.random_points(BIG - MR.CAPACITY, 8)
    far_slots = np.arange(MR.CAPACITY, BIG, dtype="i4")
    cam = S.camera()
    fr = R.synthetic_features(64, 3)

    def slp(c, t):
        with _frame(c, fr) as f:
            return Tracking.SearchLocalPoints(f, t, cam[0], S.INTR, S.SCALE, Ow=cam[1], log_scale_factor=S.LOG_SF, taps=True, ctx=c)
    with MapPointTable(BIG, ctx=ctx_b) as solo:
        solo.update(np.arange(MR.CAPACITY), **rows); solo.update(far_slots, **far)
        _refresh(solo, sc, kfs)
        want_rows = solo.fetch(sc["slot"]); want_slp = slp(ctx_b, solo)
    assert want_slp["n_to_match"] >= 100
    with MapPointTable(BIG, ctx=ctx) as root, root.attach(ctx_b) as view:
        view.update(np.arange(MR.CAPACITY), **rows)
        for _ in range(3):
            view.update(far_slots, **far)
        assert _refresh(view, sc, kfs, fetch=False) is None
        got = root.fetch(sc["slot"])
        assert all(_same(got[k], want_rows[k]) for k in COLS)
        view.update(far_slots, **far); _refresh(view, sc, kfs, fetch=False)
        assert _same(slp(ctx, root), want_slp)


# ---------------------------------------------------------------------------------------------------------------- 3. scratch per handle
def test_scratch_is_per_handle(ctx, ctx_b, world, handles_b, alone):
    w, HB = world, handles_b
    HA = Handles(ctx, w)
    with _load(MapPointTable(w["capacity"], ctx=ctx), w["rows"]) as root, root.attach(ctx_b) as view, view.attach(ctx) as second:
        assert root.handles() == 3
        for _ in range(2):                                        # interleaved: A's table, B's view, a second view in A's context
            assert _same(_slp(HA, root, w), alone["slp"])
            assert _same(_fuse(HB, view, w, R.PARAMS[0]), alone["fuse"][0])
            assert _same(_slp(HA, second, w), alone["slp"])
            assert _same(_sim3(HB, view, w), alone["sim3"])
            assert _same(_slp(HA, root, w), alone["slp"])
            assert _same(_loop(HB, view, w), alone["loop"])
            assert _same(_fuse(HB, view, w, R.PARAMS[1]), alone["fuse"][1])
        everything = np.arange(w["capacity"])
        seen = [t.fetch(everything)["seen"] for t in (root, second, view)]
        held = w["track_ids"][w["track_ids"] >= 0]
        assert (seen[0][held] == 4).all() and seen[0].max() == 4                  # the stamp of each handle's own last SearchLocalPoints
        assert (seen[1][held] == 2).all() and seen[1].max() == 2
        assert (seen[2] == 0).all()                                               # never searched through
        assert ((seen[0] == 4) == (seen[1] == 2)).all()
        second.set_order(w["order"][:20])                         # an order on one view leaves the other handles' visits alone
        cut = _slp(HA, second, w)
        assert cut["n_to_match"] < alone["slp"]["n_to_match"] and set(cut["in_view_slot"]) <= set(w["order"][:20].tolist())
        assert _same(_slp(HA, root, w), alone["slp"])
        view.set_order(w["order"][:5])
        assert _same(_slp(HA, root, w), alone["slp"]) and _same(_slp(HA, second, w), cut)
        assert _same(_all_rows(view), alone["rows"])
    HA.close()


# ---------------------------------------------------------------------------------------------------------------- 4. lifetime
def _code(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except _lib.CcmError as e:
        return e.code
    return 0


def test_lifetime_of_rows_handles_and_contexts():
    lib = _lib.load()
    ca, cb, cc = _lib.Context(0), _lib.Context(0), _lib.Context(0)
    rows = S.random_points(65, 2)
    slots = np.arange(65, dtype="i4")
    t = MapPointTable(65, ctx=ca)
    t.update(slots, **rows)
    assert t.handles() == 1
    v = t.attach(cb)
    assert t.handles() == v.handles() == 2
    w = v.attach(cc)                                              # a view of a view
    assert t.handles() == v.handles() == w.handles() == 3
    x = t.attach(ca)                                              # in the owner's own context
    assert x.handles() == 4 and _same(_all_rows(x), {k: rows[k] for k in COLS})
    x.close()
    assert t.handles() == 3
    for c, h in ((ca, v), (cb, t), (cc, v), (ca, w)):             # a handle named with a foreign context
        assert lib.ccm_map_table_set_order(c.handle, C.c_void_p(h.handle), 0, None) == E_ARG
        assert lib.ccm_map_table_fetch(c.handle, C.c_void_p(h.handle), 1, _lib.ptr(slots), *[None] * 7) == E_ARG
    out = C.c_void_p(1)
    assert lib.ccm_map_table_attach(None, C.c_void_p(t.handle), C.byref(out)) == E_ARG and out.value is None

    t.close()                                                     # the first table goes: the views keep the rows
    assert v.handles() == w.handles() == 2
    assert _same(_all_rows(v), {k: rows[k] for k in COLS})
    v.update(slots[:3], pos=np.full((3, 3), 7.0, "f4"))
    assert (w.fetch(slots[:3])["pos"] == 7.0).all()
    ca.close()                                                    # the owner's context goes
    w.update(slots[3:5], pos=np.full((2, 3), 8.0, "f4"))
    assert (v.fetch(slots[:5])["pos"] == np.repeat([7.0, 8.0], [3, 2])[:, None]).all()

    f = DeviceFrame(_view(R.synthetic_features(16, 1)), None, ctx=cc)
    cb.close()                                                    # the view's context goes: v is an orphan
    assert v.handles() == 0 and w.handles() == 1 and lib.ccm_map_table_capacity(C.c_void_p(v.handle)) == 65
    v.ctx = cc                                                    # any living context: the orphan answers before the owner is compared
    cam = S.camera()
    assert _code(v.update, slots[:1], pos=np.zeros((1, 3), "f4")) == E_STATE
    assert _code(v.set_order, slots[:2]) == E_STATE and _code(v.set_order, None) == E_STATE
    assert _code(v.fetch, slots[:1]) == E_STATE
    assert _code(v.refresh, slots[:1], [f], [0, 0], [], [], what=1) == E_STATE
    assert _code(Tracking.SearchLocalPoints, f, v, cam[0], S.INTR, S.SCALE, Ow=cam[1], ctx=cc) == E_STATE
    assert _code(Tracking.PoseOptimizationTable, f, v, np.zeros(7), np.array(S.INTR, "f8"), R.INV_SIGMA2, ctx=cc) == E_STATE
    with DeviceFrame(_view(R.synthetic_features(16, 2)), None, ctx=cc) as g:
        assert _code(Tracking.TrackWithMotionModel, f, g, v, cam[0], np.zeros(7), np.array(S.INTR, "f8"), S.SCALE, R.INV_SIGMA2, check_ori=False, ctx=cc) == E_STATE
    vp = C.c_void_p(v.handle)
    assert lib.ccm_fuse_select_table_frames(cc.handle, vp, C.byref(_lib.FuseTableProblem()), C.byref(_lib.FuseTableResult())) == E_STATE
    assert lib.ccm_search_by_sim3_table_frames(cc.handle, vp, C.byref(_lib.Sim3SearchProblem()), C.byref(_lib.Sim3SearchResult())) == E_STATE
    assert lib.ccm_search_by_projection_table_frames(cc.handle, vp, C.byref(_lib.LoopProjectionProblem()), C.byref(_lib.LoopProjectionResult())) == E_STATE
    out = C.c_void_p(1)
    assert lib.ccm_map_table_attach(cc.handle, vp, C.byref(out)) == E_STATE and out.value is None
    res = Tracking.SearchLocalPoints(f, w, cam[0], S.INTR, S.SCALE, Ow=cam[1], log_scale_factor=S.LOG_SF, ctx=cc)        # the last handle works
    assert res["n_to_match"] >= 1 and (w.fetch(slots[:5])["pos"] == np.repeat([7.0, 8.0], [3, 2])[:, None]).all()
    v.close(); f.close(); w.close(); cc.close()


# ---------------------------------------------------------------------------------------------------------------- 5. / 6. two threads
def _threads(*bodies):
    """Runs the bodies on a thread each, at once; a thread that is still alive after JOIN_S fails the test, an exception is re-raised."""
    errors = []
    start = threading.Barrier(len(bodies))

    def wrap(fn):
        def run():
            try:
                start.wait(JOIN_S)
                fn()
            except BaseException as e:  # noqa: BLE001
                errors.append(e)
        return run
    ts = [threading.Thread(target=wrap(b), daemon=True) for b in bodies]
    for t in ts:
        t.start()
    for t in ts:
        t.join(JOIN_S)
    assert not any(t.is_alive() for t in ts), "a thread did not finish within %g s" % JOIN_S
    if errors:
        raise errors[0]


N_ITER = 40


def test_two_threads_on_disjoint_rows(ctx, ctx_b, world, refresh_world):
    """Thread A tracks (SearchLocalPoints and the pose, its order restricted to R1 = the world's rows) on the table while thread B
    refreshes and fuses on R2 = the refresh scene's rows through a view; ctypes releases the GIL during the calls.  Every result of
    every iteration and the rows at the end equal the serial run's."""
    w = world
    sc, rrows, kfs = refresh_world
    off = MR.CAPACITY                                             # R2 = [0, off), R1 = [off, off + the world)
    HA = Handles(ctx, w)
    order = (w["order"] + off).astype("i4")
    ids = np.where(w["track_ids"] >= 0, w["track_ids"] + off, -1).astype("i4")
    kf0 = w["loop"]["kfs"][0]
    fuse_slots = sc["slot"][:65]
    mb = ORBmatcher(ctx=ctx_b)
    poses = [(k["Tcw"], k["Ow"]) for k in sc["kfs"][:2]]

    def track(t, out):
        for _ in range(N_ITER):
            HA.track.map_points = ids
            s = Tracking.SearchLocalPoints(HA.track, t, kf0["Tcw"], R.INTR, R.SCALE, Ow=kf0["Ow"], th=3.0, log_scale_factor=R.LOG_SF, taps=True, ctx=ctx)
            out.append((s, Tracking.PoseOptimizationTable(HA.track, t, _pose7(kf0["Tcw"]), np.array(R.INTR, "f8"), R.INV_SIGMA2, ctx=ctx)))

    def mapping(t, out):
        for i in range(N_ITER):
            r = _refresh(t, sc, kfs, pos=(sc["pos"] + np.float32(0.001 * i)).astype("f4"), fetch=bool(i % 2))
            f = mb.FuseSelectTableFrames(t, kfs[:2], [p[0] for p in poses], [p[1] for p in poses], MR.INTR, R.BOUNDS, fuse_slots, R.SCALE, R.INV_SIGMA2,
                                         log_scale_factor=R.LOG_SF, taps=True, **R.PARAMS[i % 2])
            out.append((r, f))
    with MapPointTable(off + w["capacity"], ctx=ctx) as root, root.attach(ctx_b) as view:
        root.update(np.arange(off), **rrows)
        live = np.flatnonzero(w["rows"]["flags"] & R.LIVE)
        root.update(live + off, **{k: w["rows"][k][live] for k in COLS})
        root.set_order(order)
        sa, sb, ta, tb = [], [], [], []
        track(root, sa); mapping(view, sb)                        # the serial run
        serial_rows = _all_rows(root)
        assert sa[0][0]["n_to_match"] >= 20 and not _same(sb[0][1], sb[2][1])     # the mapping thread's results move with its writes
        _threads(lambda: track(root, ta), lambda: mapping(view, tb))
        assert len(ta) == len(tb) == N_ITER
        for i in range(N_ITER):
            assert _same(ta[i], sa[i]), ("tracking", i)
            assert _same(tb[i], sb[i]), ("mapping", i)
        assert _same(_all_rows(root), serial_rows) and _same(_all_rows(view), serial_rows)
    HA.close()


def test_two_threads_on_the_same_rows_see_whole_updates(ctx, ctx_b):
    """B writes pos = iteration into all of R2 with N_ITER updates that do not synchronise while A fetches R2 again and again: one fetch
    never sees two iterations, and the iteration never goes back.  The iteration count is fixed."""
    n = 20000
    r2 = np.arange(n, dtype="i4")
    seen_values = []
    done = threading.Event()
    with MapPointTable(n, ctx=ctx) as root, root.attach(ctx_b) as view:
        root.update(r2, pos=np.full((n, 3), -1.0, "f4"), flags=np.full(n, 1, np.uint8))

        def writer():
            try:
                for i in range(N_ITER):
                    view.update(r2, pos=np.full((n, 3), float(i), "f4"))
            finally:
                done.set()

        def reader():
            while not done.is_set() and len(seen_values) < 100000:
                seen_values.append(np.unique(root.fetch(r2)["pos"]))
            seen_values.append(np.unique(root.fetch(r2)["pos"]))
        _threads(writer, reader)
    assert all(len(u) == 1 for u in seen_values), [u for u in seen_values if len(u) != 1][:3]
    v = np.array([u[0] for u in seen_values])
    assert (np.diff(v) >= 0).all() and v[-1] == N_ITER - 1 and v[0] >= -1
    print("%d fetches while %d updates ran, %d distinct iterations seen" % (len(v), N_ITER, len(np.unique(v))))
