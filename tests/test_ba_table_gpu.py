"""ccm_ba_solve_table_frames on the GPU (include/ccm_hot.h "local BA on the table").  The contract is bit equality with ccm_ba_solve on
the array problem the same data gives by widening (tests/ba_table_case.py builds both): the two routes run in the same process on the
same context, the same LM kernels produce both sides, and the table route's two own kernels only move values whose conversions are
exact (float -> double) or defined (double -> float, one rounding).  Every comparison is therefore `==` on bytes; the array route is
held to the CPU oracle by the bound of test_ba_gpu.py (pose delta 1e-5, same iteration and trial counts)."""
import numpy as np
import pytest

import ba_table_case as B
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd._lib import MPR_NORMAL_DEPTH
from motioncheck_ccm_slam_amd.optimizer import Optimizer, pose_delta, pose_to_camera

pytestmark = pytest.mark.gpu
TOL = 1e-5
SCALARS = ("iterations_done", "trials", "chi2_initial", "chi2_final", "lambda_final", "stopped", "schur_blocks", "schur_pairs",
           "pcg_iterations", "pcg_fallbacks", "pcg_pipelined")
_cache = {}


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _graph(name):
    if name == "reduced":
        return B.reduced(B.graph("small"))
    if name == "empty":
        return B.with_empty_point(B.graph("small"))
    return B.graph(name)


def _solved(ctx, name):
    """One graph through both routes, LocalBundleAdjustmentClient's schedule: (lists, case, rows before, array result, table result,
    rows after, handle poses after).  Computed once per graph and left unchanged."""
    if name not in _cache:
        Lst = B.lists(_graph(name))
        case = B.Case(ctx, Lst)
        before = case.rows()
        ra = Optimizer.LocalBundleAdjustmentClient(Lst["arrays"], ctx=ctx)
        rt = Optimizer.LocalBundleAdjustmentClientTable(case.table, case.kfs, Lst["table_lists"], ctx=ctx)
        after = case.rows()
        cams = [h.pose() for h in case.kfs]
        _cache[name] = (Lst, case, before, ra, rt, after, cams)
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for v in _cache.values():
        v[1].close()
    _cache.clear()


def _check_routes_agree(Lst, before, ra, rt, after):
    assert _bits(rt["poses"], ra["poses"])
    assert _bits(rt["outlier"], ra["outlier"])
    for k in SCALARS:
        assert rt[k] == ra[k], k
    want = ra["points"].astype("f4")
    slot = Lst["slot"]
    assert _bits(rt["pos"], want) and _bits(after["pos"][slot], want)
    # the rows outside the list, and the other columns of the listed rows, are as they were
    rest = np.ones(Lst["capacity"], bool); rest[slot] = False
    for k in B.COLS:
        assert _bits(after[k][rest], before[k][rest]), k
        if k != "pos":
            assert _bits(after[k][slot], before[k][slot]), k


def test_config4_local_ba_schedule(ctx, oracle):
    Lst, case, before, ra, rt, after, _ = _solved(ctx, "config4")
    assert ra["outlier"].sum() > 0 and ra["iterations_done"] > 0
    _check_routes_agree(Lst, before, ra, rt, after)
    assert not _bits(after["pos"][Lst["slot"]], before["pos"][Lst["slot"]])        # the solve moved the points
    # the array route itself meets the oracle bound of test_local_ba_config4
    ref = oracle.ba_solve(Lst["arrays"], 5, float(np.float32(np.sqrt(5.991))), 10)
    assert pose_delta(ra["poses"], ref["poses"]).max() <= TOL
    assert ra["iterations_done"] == ref["iterations_done"] and ra["trials"] == ref["trials"]


@pytest.mark.parametrize("name", ["small", "wave", "block", "long", "reduced", "empty"])
def test_small_graphs_both_schedules(ctx, name):
    Lst, case, before, ra, rt, after, _ = _solved(ctx, name)
    if name == "empty":                                              # landmark 1 is a vertex without edges, and its row is still written
        assert Lst["obs_first"][1] == Lst["obs_first"][2] and (np.diff(Lst["obs_first"]) > 0).sum() == Lst["L"] - 1
    _check_routes_agree(Lst, before, ra, rt, after)
    # BundleAdjustmentClient's schedule on a case of its own: 5 iterations, no second stage, no outlier output
    c2 = B.Case(ctx, Lst)
    try:
        b0 = c2.rows()
        ga = Optimizer.BundleAdjustmentClient(Lst["arrays"], 5, ctx=ctx)
        gt = Optimizer.BundleAdjustmentClientTable(c2.table, c2.kfs, Lst["table_lists"], 5, ctx=ctx)
        assert gt["outlier"] is None and ga["outlier"] is None
        gt["outlier"] = ga["outlier"] = np.zeros(0, np.uint8)
        _check_routes_agree(Lst, b0, ga, gt, c2.rows())
    finally:
        c2.close()


@pytest.mark.parametrize("name", ["small", "reduced"])
def test_publish_and_refresh(ctx, name):
    Lst, _, before, ra, _, _, _ = _solved(ctx, name)
    case = B.Case(ctx, Lst)                                          # a case of its own: the refresh below writes its table
    try:
        _publish_and_refresh(ctx, Lst, case, before, ra)
    finally:
        case.close()


def _publish_and_refresh(ctx, Lst, case, before, ra):
    rt = Optimizer.LocalBundleAdjustmentClientTable(case.table, case.kfs, Lst["table_lists"], ctx=ctx)
    cams = [h.pose() for h in case.kfs]
    pub = Lst["publish"].astype(bool)
    assert pub.any() and (~pub).any() and _bits(rt["poses"], ra["poses"])
    for k in range(Lst["P"]):
        T, O = cams[k]
        if pub[k]:
            Tw, Ow = pose_to_camera(rt["poses"][k])
            assert _bits(T, Tw) and _bits(O, Ow), k
        else:
            assert _bits(T, case.cams[k][0]) and _bits(O, case.cams[k][1]), k
    assert any(not _bits(cams[k][0], case.cams[k][0]) for k in np.flatnonzero(pub))      # a published pose did move
    # UpdateNormalAndDepth from the device-side results == the same from results sent up by update / set_pose
    args = (Lst["slot"], None, Lst["obs_first"], Lst["obs_kf"], Lst["obs_feat"], Lst["ref_kf"], Lst["ref_feat"])
    got = case.table.refresh(args[0], case.kfs, *args[2:], pos=None, what=MPR_NORMAL_DEPTH)
    rows_a = case.rows()
    poses_b = np.where(pub[:, None], ra["poses"], Lst["arrays"]["poses"])
    c2 = B.Case(ctx, Lst, poses=poses_b)
    try:
        c2.table.update(Lst["slot"], pos=ra["points"].astype("f4"))
        want = c2.table.refresh(args[0], c2.kfs, *args[2:], pos=None, what=MPR_NORMAL_DEPTH)
        rows_b = c2.rows()
    finally:
        c2.close()
    for k in want:
        assert _bits(got[k], want[k]), k
    for k in B.COLS:
        assert _bits(rows_a[k], rows_b[k]), k
    assert not _bits(rows_a["normal"][Lst["slot"]], before["normal"][Lst["slot"]])


def test_publish_into_a_handle_without_a_keyframe_block(ctx):
    """A published handle that never had a camera or a pose gets its keyframe block from the call; the device copy and the handle's
    host copy hold the same bits, which a later set_camera -- it uploads the whole host copy -- must not change."""
    Lst, _, _, ra, _, _, _ = _solved(ctx, "wave")
    j = int(np.flatnonzero(Lst["publish"])[0])
    case = B.Case(ctx, Lst, bare=(j,))
    try:
        with pytest.raises(_lib.CcmError) as ei:
            case.kfs[j].pose()
        assert ei.value.code == -7                                   # CCM_E_STATE: no pose yet
        rt = Optimizer.LocalBundleAdjustmentClientTable(case.table, case.kfs, Lst["table_lists"], ctx=ctx)
        assert _bits(rt["poses"], ra["poses"]) and _bits(rt["outlier"], ra["outlier"]) and _bits(rt["pos"], ra["points"].astype("f4"))
        Tw, Ow = pose_to_camera(rt["poses"][j])
        T, O = case.kfs[j].pose()
        assert _bits(T, Tw) and _bits(O, Ow)
        case.kfs[j].set_camera([float(np.float32(v)) for v in Lst["arrays"]["intr"][j]], B.SCALE, B.SIGMA2)
        T, O = case.kfs[j].pose()
        assert _bits(T, Tw) and _bits(O, Ow)
        # the same for a handle that had both: its host copy follows the device
        k = int(np.flatnonzero(Lst["publish"])[-1])
        assert k != j
        case.kfs[k].set_camera([float(np.float32(v)) for v in Lst["arrays"]["intr"][k]], B.SCALE, B.SIGMA2)
        T, O = case.kfs[k].pose()
        Tw, Ow = pose_to_camera(rt["poses"][k])
        assert _bits(T, Tw) and _bits(O, Ow)
    finally:
        case.close()


def test_state_errors(ctx):
    """CCM_E_STATE: a communicator of more than one rank (the table route is unsharded), a table and a handle that outlived their
    context.  The table is untouched each time."""
    import ctypes as C
    from motioncheck_ccm_slam_amd.frame import DeviceFrame
    from motioncheck_ccm_slam_amd.matcher import FrameGridView
    from motioncheck_ccm_slam_amd.tracking import MapPointTable
    Lst = B.lists(_graph("wave"))

    class Transport(C.Structure):                                    # ccm_comm_transport
        _fields_ = [("user", C.c_void_p), ("allreduce_f64", C.c_void_p), ("allreduce_u8_max", C.c_void_p), ("destroy", C.c_void_p)]
    f64 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)(lambda *a: 1)     # never called: the answer comes first
    u8 = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)(lambda *a: 1)
    tr = Transport(None, C.cast(f64, C.c_void_p), C.cast(u8, C.c_void_p), None)
    other = _lib.Context(0)
    case = None
    try:
        case = B.Case(other, Lst)
        before = case.rows()
        other.check(other.lib.ccm_comm_attach(other.handle, C.byref(tr), 2, 0))
        try:
            with pytest.raises(_lib.CcmError) as ei:
                Optimizer.LocalBundleAdjustmentClientTable(case.table, case.kfs, Lst["table_lists"], ctx=other)
            assert ei.value.code == -7
        finally:
            other.check(other.lib.ccm_comm_destroy(other.handle))
        after = case.rows()
        for k in B.COLS:
            assert _bits(after[k], before[k]), k
        r = Optimizer.LocalBundleAdjustmentClientTable(case.table, case.kfs, Lst["table_lists"], ctx=other)      # one rank again: it works
        assert r["iterations_done"] > 0
        case.close(); case = None
        orphan_t = MapPointTable(Lst["capacity"], ctx=other)
        f0 = Lst["feats"][0]
        orphan_f = DeviceFrame(FrameGridView(f0["kx"], f0["ky"], f0["oct"], f0["desc"]), None, ctx=other)
    finally:
        if case is not None:
            case.close()
        other.close()
    mine = B.Case(ctx, Lst)                                          # the other context is gone
    try:
        before = mine.rows()
        for table, kfs in ((orphan_t, mine.kfs), (mine.table, [orphan_f] + mine.kfs[1:])):
            with pytest.raises(_lib.CcmError) as ei:
                Optimizer.LocalBundleAdjustmentClientTable(table, kfs, Lst["table_lists"], ctx=ctx)
            assert ei.value.code == -7
        after = mine.rows()
        for k in B.COLS:
            assert _bits(after[k], before[k]), k
    finally:
        mine.close()
        orphan_t.close(); orphan_f.close()


def test_stop_flag_up_on_entry(ctx):
    Lst = B.lists(_graph("small"))
    case = B.Case(ctx, Lst)
    try:
        before = case.rows()
        r = Optimizer.LocalBundleAdjustmentClientTable(case.table, case.kfs, Lst["table_lists"], pbStopFlag=np.ones(1, np.uint8), ctx=ctx)
        assert r["stopped"] and r["iterations_done"] == 0
        assert _bits(r["poses"], Lst["arrays"]["poses"])
        after = case.rows()
        for k in B.COLS:
            assert _bits(after[k], before[k]), k
        assert _bits(r["pos"], before["pos"][Lst["slot"]])
        for k, h in enumerate(case.kfs):
            T, O = h.pose()
            assert _bits(T, case.cams[k][0]) and _bits(O, case.cams[k][1]), k
    finally:
        case.close()


def test_errors_leave_the_table_untouched(ctx):
    Lst = B.lists(_graph("wave"))
    case = B.Case(ctx, Lst)
    other = _lib.Context(0)
    foreign = None
    try:
        from motioncheck_ccm_slam_amd.tracking import MapPointTable
        foreign = MapPointTable(Lst["capacity"], ctx=other)
        before = case.rows()
        base = Lst["table_lists"]
        e0 = 0                                                       # list entry 0: keyframe obs_kf[0], feature obs_feat[0]

        def variant(**kw):
            d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
            d.update(kw)
            return d
        slot2 = base["slot"].copy(); slot2[1] = slot2[0]
        feat2 = base["obs_feat"].copy(); feat2[e0] = case.kfs[int(base["obs_kf"][e0])].n
        kf2 = base["obs_kf"].copy(); kf2[e0] = Lst["P"]
        top = max(int(f["oct"].max()) for f in Lst["feats"]) + 1     # the largest n_levels among the handles
        bad = [
            ("slot twice", case.table, case.kfs, variant(slot=slot2)),
            ("handle twice", case.table, [case.kfs[0]] + case.kfs[:-1], base),
            ("feature == N", case.table, case.kfs, variant(obs_feat=feat2)),
            ("keyframe == n_kf", case.table, case.kfs, variant(obs_kf=kf2)),
            ("n_levels too small", case.table, case.kfs, variant(inv_level_sigma2=B.INV_SIGMA2[:top - 1])),
            ("table of another context", foreign, case.kfs, base),
        ]
        for what, table, kfs, lists in bad:
            with pytest.raises(_lib.CcmError) as ei:
                Optimizer.LocalBundleAdjustmentClientTable(table, kfs, lists, ctx=ctx)
            assert ei.value.code == -1, what                         # CCM_E_ARG
            after = case.rows()
            for k in B.COLS:
                assert _bits(after[k], before[k]), (what, k)
        for k, h in enumerate(case.kfs):                             # and the handles kept their poses
            T, O = h.pose()
            assert _bits(T, case.cams[k][0]) and _bits(O, case.cams[k][1]), k
    finally:
        if foreign is not None:
            foreign.close()
        case.close()
        other.close()


def test_call_through_a_table_view(ctx):
    """The solve runs in a second context through its view of the table, with that context's own handles; the root handle's fetch,
    a call that starts after the solve has returned, sees the new positions."""
    Lst, _, _, ra, _, _, _ = _solved(ctx, "small")
    from motioncheck_ccm_slam_amd.tracking import MapPointTable
    ctx2 = _lib.Context(0)
    root = MapPointTable(Lst["capacity"], ctx=ctx)
    view = None; case2 = None
    try:
        root.update(np.arange(Lst["capacity"], dtype="i4"), **Lst["rows"])
        view = root.attach(ctx2)
        case2 = B.Case(ctx2, Lst, table=view, load=False)
        r = Optimizer.LocalBundleAdjustmentClientTable(view, case2.kfs, Lst["table_lists"], ctx=ctx2)
        got = root.fetch(Lst["slot"])
        assert _bits(r["poses"], ra["poses"]) and _bits(r["outlier"], ra["outlier"])
        assert _bits(got["pos"], ra["points"].astype("f4")) and _bits(r["pos"], got["pos"])
    finally:
        if case2 is not None:
            case2.close()
        if view is not None:
            view.close()
        root.close()
        ctx2.close()
