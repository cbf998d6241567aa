"""ccm_map_table_refresh on the GPU: MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth for a list of map
points read from keyframe handles, against the numpy restatement tests/map_refresh_ref.py bit for bit (every observation count of
its scene, ties, a point on a camera centre, a list longer than the kernel's LDS copy), against the old route's descriptor choice,
column selection, positions and flags given in the call, the form that does not synchronise, SearchLocalPoints afterwards, misuse
and a repeated call.  Every out-of-range case is refused on the host."""
import ctypes as C

import numpy as np
import pytest

import map_refresh_ref as R
import search_local_points_ref as SLP
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.matcher import FrameGridView
from motioncheck_ccm_slam_amd.tracking import MapPointTable, Tracking
from motioncheck_ccm_slam_amd.vocabulary import ORBVocabulary, synthetic_tree

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -7
COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")
K = np.array(R.INTR, "f4")


def _handle(ctx, kf, camera=True, pose=True):
    h = DeviceFrame(FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"]), None, ctx=ctx)
    if camera:
        h.set_camera(K, kf["sf"], kf["sigma2"])
    if pose:
        h.set_pose(kf["Tcw"], kf["Ow"])
    return h


@pytest.fixture(scope="module")
def world(ctx):
    """The scene, its keyframe handles, the rows a table holds before the call (positions already sent) and the numpy reference of
    the full call; computed once and left unchanged."""
    S = R.scene(1)
    rows = R.table_rows(2)
    rows["pos"][S["slot"]] = S["pos"]
    ref = R.refresh(S, {k: v[S["slot"]] for k, v in rows.items()}, 3)
    kfs = [_handle(ctx, kf) for kf in S["kfs"]]
    yield S, rows, ref, kfs
    for h in kfs:
        h.close()


def _table(ctx, rows):
    t = MapPointTable(R.CAPACITY, ctx=ctx)
    t.update(np.arange(R.CAPACITY), **{k: rows[k] for k in COLS})
    return t


def _refresh(t, S, kfs, **kw):
    return t.refresh(S["slot"], kfs, S["obs_first"], S["obs_kf"], S["obs_feat"], S["ref_kf"], S["ref_feat"], **kw)


def _same_floats(a, b):
    """Bit-equal, with NaN in the same places (the payload of a NaN is not compared)."""
    a = np.ascontiguousarray(a, "f4"); b = np.ascontiguousarray(b, "f4")
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and (na == nb).all() and (a.view("u4")[~na] == b.view("u4")[~na]).all()


def _rows_equal(got, want, cols=("normal", "min_dist", "max_dist", "desc")):
    return all(_same_floats(got[k], want[k]) if k != "desc" and k != "flags" else (got[k] == want[k]).all() for k in cols)


def _check_table(t, S, rows, ref, cols=("pos", "normal", "min_dist", "max_dist", "desc")):
    """The listed slots hold the reference's rows, every other slot what it held before."""
    all_rows = t.fetch(np.arange(R.CAPACITY))
    listed = np.zeros(R.CAPACITY, bool); listed[S["slot"]] = True
    for k in COLS:
        assert (all_rows[k][~listed].view(np.uint8) == rows[k][~listed].view(np.uint8)).all(), k
    got = {k: all_rows[k][S["slot"]] for k in COLS}
    assert _rows_equal(got, ref, cols)
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. parity
def test_parity_with_the_restatement_and_the_old_route(ctx, world):
    S, rows, ref, kfs = world
    with _table(ctx, rows) as t:
        out = _refresh(t, S, kfs)
        assert (out["best"] == ref["best"]).all()
        assert _rows_equal(out, ref, ("normal", "min_dist", "max_dist"))
        nan = np.isnan(out["normal"]).any(1)
        assert nan.sum() == 1 and nan[S["on_centre"]]
        got = _check_table(t, S, rows, ref)
        empty = S["counts"] == 0                                  # both functions return early: the row stays, best = -1
        before = {k: rows[k][S["slot"]] for k in COLS}
        assert empty.sum() >= 10 and (out["best"][empty] == -1).all() and (out["best"][~empty] >= 0).all()
        for k in COLS:
            assert (got[k][empty].view(np.uint8) == before[k][empty].view(np.uint8)).all(), k
        assert (got["flags"] == before["flags"]).all()
    g, first, count = R.gathered_descriptors(S)                   # the old route: host gather, ccm_distinctive_descriptors
    par, desc, w = synthetic_tree(3, 2, seed=1, ragged=False)
    old = ORBVocabulary(3, 2, par, desc, w, ctx=ctx).distinctive_descriptors(g, first, count)
    assert (old == out["best"]).all()
    assert (out["best"][S["counts"] == 300] >= 0).all() and ref["tie"][S["counts"] >= 3].mean() >= 0.2


# ---------------------------------------------------------------------------------------------------------------- 2. columns
def test_column_selection(ctx, world):
    S, rows, ref, kfs = world
    before = {k: rows[k][S["slot"]] for k in COLS}
    with _table(ctx, rows) as t:                                  # the descriptor alone
        out = _refresh(t, S, kfs, what=R.DESCRIPTOR)
        assert (out["best"] == ref["best"]).all()
        mixed = dict(before, desc=ref["desc"])
        _check_table(t, S, rows, mixed)
        assert _rows_equal(out, before, ("normal", "min_dist", "max_dist"))     # the result reports the rows as they stand
    with _table(ctx, rows) as t:                                  # normal and depth alone: best comes back -1
        out = _refresh(t, S, kfs, what=R.NORMAL_DEPTH)
        assert (out["best"] == -1).all()
        mixed = dict(ref, desc=before["desc"])
        _check_table(t, S, rows, mixed)
        assert _rows_equal(out, ref, ("normal", "min_dist", "max_dist"))


# ---------------------------------------------------------------------------------------------------------------- 3. positions
def test_positions_and_flags_given_in_the_call(ctx, world):
    S, rows, ref, kfs = world
    stale = R.table_rows(2)                                       # the table holds other positions for the listed slots
    assert (stale["pos"][S["slot"]] != S["pos"]).any()
    flags = (np.arange(len(S["slot"])) % 8).astype(np.uint8)
    with _table(ctx, stale) as t:
        out = _refresh(t, S, kfs, pos=S["pos"], flags=flags)
        assert (out["best"] == ref["best"]).all() and _rows_equal(out, ref, ("normal", "min_dist", "max_dist"))
        got = _check_table(t, S, stale, ref)
        assert (got["pos"].view("u4") == S["pos"].view("u4")).all() and (got["flags"] == flags).all()   # also where c == 0


# ---------------------------------------------------------------------------------------------------------------- 4. no sync
def test_form_without_download(ctx, world):
    S, rows, ref, kfs = world
    with _table(ctx, rows) as t:
        assert _refresh(t, S, kfs, fetch=False) is None
        _check_table(t, S, rows, ref)


# ---------------------------------------------------------------------------------------------------------------- 5. downstream
def test_search_local_points_sees_the_refreshed_rows(ctx, world):
    S, rows, ref, kfs = world
    T, Ow = SLP.camera(rotvec=(0.03, -0.05, 0.02), t=(0.0, 0.0, 4.0))
    ok = (S["counts"] > 0) & ~np.isnan(ref["normal"]).any(1)
    sub = np.flatnonzero(ok)[:200]
    fr = SLP.frustum(S["pos"][sub], ref["normal"][sub], ref["min_dist"][sub], ref["max_dist"][sub], T, Ow)
    vis = fr["gate"] == 0
    assert vis.sum() >= 100
    view = FrameGridView(fr["u"][vis], fr["v"][vis], fr["level"][vis], ref["desc"][sub][vis])
    want_rows = {k: rows[k].copy() for k in COLS}
    for k in ("normal", "min_dist", "max_dist", "desc"):
        want_rows[k][S["slot"]] = ref[k]
    res = []
    for via_refresh in (True, False):
        with _table(ctx, rows if via_refresh else want_rows) as t, DeviceFrame(view, None, ctx=ctx) as f:
            if via_refresh:
                _refresh(t, S, kfs, fetch=False)
            res.append(Tracking.SearchLocalPoints(f, t, T, SLP.INTR, SLP.SCALE, Ow=Ow, log_scale_factor=SLP.LOG_SF, taps=True))
    a, b = res
    assert a["nmatches"] == b["nmatches"] and a["n_to_match"] == b["n_to_match"] >= 100 and a["nmatches"] >= 1
    for k in ("match", "mp_id", "in_view_slot", "level", "occupied"):
        assert (a[k] == b[k]).all(), k
    print("downstream: %d in view, %d matches" % (a["n_to_match"], a["nmatches"]))


# ---------------------------------------------------------------------------------------------------------------- 6. errors
def _raw(ctx, t, kfs, slot, first, okf, ofeat, rkf, rfeat, what, outs):
    a = lambda v: np.ascontiguousarray(v, "i4")  # noqa: E731
    slot, first, okf, ofeat, rkf, rfeat = [a(v) for v in (slot, first, okf, ofeat, rkf, rfeat)]
    handles = (C.c_void_p * max(len(kfs), 1))(*[k.handle for k in kfs])
    u = _lib.MapRefresh(len(slot), _lib.ptr(slot), None, None, len(kfs), handles, _lib.ptr(first), _lib.ptr(okf), _lib.ptr(ofeat),
                        _lib.ptr(rkf), _lib.ptr(rfeat), what)
    r = _lib.MapRefreshResult(*[_lib.ptr(outs[k]) for k in ("best", "normal", "min_dist", "max_dist")])
    return ctx.lib.ccm_map_table_refresh(ctx.handle, C.c_void_p(t.handle), C.byref(u), C.byref(r))


def test_errors_leave_table_and_outputs_untouched(ctx, world):
    S, rows, ref, kfs = world
    kf0 = S["kfs"][0]
    # two points: the first sees features 5 and 6 of kfs[0] and 7 of kfs[1], the second feature 8 of kfs[1]
    good = dict(slot=[3, 9], first=[0, 3, 4], okf=[0, 0, 1, 1], ofeat=[5, 6, 7, 8], rkf=[0, 1], rfeat=[5, 8])
    other = _lib.Context(0)
    try:
        with _table(ctx, rows) as t, _handle(ctx, kf0, pose=False) as no_pose, _handle(ctx, kf0, camera=False) as no_cam, \
                _handle(ctx, kf0, camera=False, pose=False) as bare, _handle(other, kf0) as foreign:
            def outs():
                return dict(best=np.full(2, 77, "i4"), normal=np.full((2, 3), 77, "f4"), min_dist=np.full(2, 77, "f4"), max_dist=np.full(2, 77, "f4"))

            def refused(code, what=3, kfl=None, **change):
                o = outs()
                rc = _raw(ctx, t, kfs[:2] if kfl is None else kfl, what=what, outs=o, **dict(good, **change))
                assert rc == code, (rc, change, ctx.lib.ccm_last_error(ctx.handle))
                assert all((v == 77).all() for v in o.values())
                got = t.fetch(np.arange(R.CAPACITY))
                for k in COLS:
                    assert (got[k].view(np.uint8) == rows[k].view(np.uint8)).all(), k
            refused(E_ARG, slot=[3, R.CAPACITY])                  # a slot out of range
            refused(E_ARG, slot=[3, -1])
            refused(E_ARG, slot=[3, 3])                           # a slot twice
            refused(E_ARG, first=[0, 3, 2])                       # obs_first descending
            refused(E_ARG, first=[1, 3, 4])                       # not from 0
            refused(E_ARG, okf=[0, 0, 2, 1])                      # a keyframe index equal to n_kf
            refused(E_ARG, ofeat=[5, 300, 7, 8])                  # a feature index equal to N
            assert b"point 0" in ctx.lib.ccm_last_error(ctx.handle) and b"entry 1" in ctx.lib.ccm_last_error(ctx.handle)
            refused(E_ARG, rkf=[0, 2])
            refused(E_ARG, rfeat=[300, 8])
            refused(E_ARG, what=0)
            refused(E_ARG, what=4)
            refused(E_STATE, kfl=[kfs[0], no_pose])               # an observed handle without a pose
            assert b"pose" in ctx.lib.ccm_last_error(ctx.handle)
            refused(E_STATE, kfl=[kfs[0], kfs[1], no_cam], rkf=[2, 1])        # a reference handle without a camera
            assert b"camera" in ctx.lib.ccm_last_error(ctx.handle)
            refused(E_ARG, kfl=[kfs[0], foreign])                 # a handle of a second context
            o = outs()                                            # the descriptor alone needs neither pose nor camera
            assert _raw(ctx, t, [bare, bare], what=R.DESCRIPTOR, outs=o, **good) == 0
            d = kf0["desc"]
            assert o["best"][0] == R.distinctive(d[[5, 6, 7]])[0] and o["best"][1] == 0
            assert (t.fetch([3, 9])["desc"] == d[[[5, 6, 7][o["best"][0]], 8]]).all()
            o = outs()                                            # n = 0 is OK and touches nothing
            assert _raw(ctx, t, kfs[:2], [], [0], [], [], [], [], 3, o) == 0 and all((v == 77).all() for v in o.values())
        orphan = MapPointTable(16, ctx=other)
        orphan_kf = _handle(other, kf0)
    finally:
        other.close()
    o = dict(best=np.full(2, 77, "i4"), normal=np.full((2, 3), 77, "f4"), min_dist=np.full(2, 77, "f4"), max_dist=np.full(2, 77, "f4"))
    assert _raw(ctx, orphan, kfs[:2], what=3, outs=o, **good) == E_STATE      # a table that outlived its context
    with _table(ctx, rows) as t:
        assert _raw(ctx, t, [kfs[0], orphan_kf], what=3, outs=o, **good) == E_STATE   # and a handle that did
    assert all((v == 77).all() for v in o.values())
    orphan.close(); orphan_kf.close()


# ---------------------------------------------------------------------------------------------------------------- 7. repeat
def test_repeated_call_gives_identical_results(ctx, world):
    S, rows, ref, kfs = world
    with _table(ctx, rows) as t:
        a = _refresh(t, S, kfs)
        t.fetch(np.arange(7))                                     # another user of the context's staging in between
        b = _refresh(t, S, kfs)
        for k in a:
            assert (a[k].view(np.uint8) == b[k].view(np.uint8)).all(), k
        _check_table(t, S, rows, ref)
