"""ccm_map_table_correct_frames on the GPU: the keyframe and map-point correction of a loop closure or a map merge on keyframe handles
and the map-point table, against the array route (Optimizer.CorrectMapPoints, then update, set_pose, refresh) byte for byte and
against the numpy restatement tests/map_correct_ref.py: both orders of the camera-centre rule, the rigid form, sizes on the edges of
a workgroup, the form that does not synchronise, a view on a second context, misuse and a repeated call.  Every out-of-range case is
refused on the host."""
import ctypes as C

import numpy as np
import pytest

import map_correct_ref as MC
import map_refresh_ref as R
import search_local_points_ref as SLP
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.matcher import FrameGridView
from motioncheck_ccm_slam_amd.optimizer import Optimizer, pose_to_camera
from motioncheck_ccm_slam_amd.tracking import MapPointTable, Tracking

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -7
COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")
OUT = ("pos", "normal", "min_dist", "max_dist")
K = np.array(R.INTR, "f4")


def _handle(ctx, kf, camera=True, pose=True):
    h = DeviceFrame(FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"]), None, ctx=ctx)
    if camera:
        h.set_camera(K, kf["sf"], kf["sigma2"])
    if pose:
        h.set_pose(kf["Tcw"], kf["Ow"])
    return h


def _reset(kfs, S):
    """Every handle back to the scene's pose (a call moves the first n_moved of them)."""
    for h, kf in zip(kfs, S["kfs"]):
        h.set_pose(kf["Tcw"], kf["Ow"])


@pytest.fixture(scope="module")
def world(ctx):
    """The scene, its keyframe handles and the rows a table holds before the call; the scene and the rows are left unchanged, the
    handles are reset by every test that uses them."""
    Cs = MC.scene(1)
    rows = R.table_rows(2)
    rows["pos"][Cs["S"]["slot"]] = Cs["S"]["pos"]
    kfs = [_handle(ctx, kf) for kf in Cs["S"]["kfs"]]
    yield Cs, rows, kfs
    for h in kfs:
        h.close()


def _table(ctx, rows):
    t = MapPointTable(R.CAPACITY, ctx=ctx)
    t.update(np.arange(R.CAPACITY), **{k: rows[k] for k in COLS})
    return t


def _correct(t, Cs, kfs, rigid=False, in_order=False, with_lists=True, sel=None, n_moved=None, owner=None, **kw):
    S = Cs["S"]
    nm = Cs["n_moved"] if n_moved is None else n_moved
    owner = Cs["owner"] if owner is None else owner
    sel = slice(None) if sel is None else sel
    ls = None
    if with_lists:
        first = np.concatenate([[0], np.cumsum(S["counts"][sel])]).astype("i4")
        e = np.concatenate([np.arange(a, b) for a, b in zip(S["obs_first"][:-1][sel], S["obs_first"][1:][sel])] + [np.zeros(0, "i8")]).astype("i8")
        ls = (first, S["obs_kf"][e], S["obs_feat"][e], S["ref_kf"][sel], S["ref_feat"][sel])
    tr = dict(Tcw_after=Cs["Tcw_after"][:nm], Ow_after=Cs["Ow_after"][:nm]) if rigid else dict(sim3_before=Cs["sim3_before"][:nm], sim3_after=Cs["sim3_after"][:nm])
    return t.correct(kfs, nm, S["slot"][sel], owner[sel], in_order=in_order, lists=ls, **tr, **kw)


def _same_floats(a, b):
    """Bit-equal, with NaN in the same places (the payload of a NaN is not compared)."""
    a = np.ascontiguousarray(a, "f4"); b = np.ascontiguousarray(b, "f4")
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and (na == nb).all() and (a.view("u4")[~na] == b.view("u4")[~na]).all()


def _before(Cs, rows):
    return {k: rows[k][Cs["S"]["slot"]] for k in COLS}


def _check_table(t, Cs, rows, want, sel=None):
    """The listed slots hold `want` in pos / normal / min_dist / max_dist and what they held in desc / flags, every other slot what it
    held before; the seen stamps are all as a fresh table has them."""
    slot = Cs["S"]["slot"] if sel is None else Cs["S"]["slot"][sel]
    all_rows = t.fetch(np.arange(R.CAPACITY))
    listed = np.zeros(R.CAPACITY, bool); listed[slot] = True
    for k in COLS:
        assert (all_rows[k][~listed].view(np.uint8) == rows[k][~listed].view(np.uint8)).all(), k
    assert (all_rows["seen"] == 0).all()
    got = {k: all_rows[k][slot] for k in COLS}
    for k in OUT:
        assert _same_floats(got[k], want[k]), k
    assert (got["desc"] == rows["desc"][slot]).all() and (got["flags"] == rows["flags"][slot]).all()
    return got


def _check_poses(kfs, Cs, Tcw, Ow):
    """The moved handles hold the given poses on the device, the others the scene's."""
    nm = len(Tcw)
    for k, h in enumerate(kfs):
        T, O = h.pose()
        wT, wO = (Tcw[k], Ow[k]) if k < nm else (Cs["S"]["kfs"][k]["Tcw"], Cs["S"]["kfs"][k]["Ow"])
        assert T.tobytes() == np.ascontiguousarray(wT, "f4").tobytes() and O.tobytes() == np.ascontiguousarray(wO, "f4").tobytes(), k


def _sim3_poses(Cs, nm=None):
    nm = Cs["n_moved"] if nm is None else nm
    p = [pose_to_camera(np.concatenate([s[:4], s[4:7] * (1.0 / s[7])])) for s in Cs["sim3_after"][:nm]]
    return [a for a, _ in p], [b for _, b in p]


def _old_route(ctx, t, Cs, kfs, fetch=True):
    """Today's route: the array call, the rows sent back, one set_pose per keyframe, the refresh of the points that moved."""
    S = Cs["S"]; owner = Cs["owner"]
    pos = t.fetch(S["slot"])["pos"]
    new = Optimizer.CorrectMapPoints(pos.astype("f8"), owner, Cs["sim3_before"], Cs["sim3_after"], ctx=ctx).astype("f4")
    t.update(S["slot"], pos=new)
    for k, (T, O) in enumerate(zip(*_sim3_poses(Cs))):
        kfs[k].set_pose(T, O)
    m = np.flatnonzero(owner >= 0)
    first = np.concatenate([[0], np.cumsum(S["counts"][m])]).astype("i4")
    e = np.concatenate([np.arange(a, b) for a, b in zip(S["obs_first"][:-1][m], S["obs_first"][1:][m])]).astype("i8")
    t.refresh(S["slot"][m], kfs, first, S["obs_kf"][e], S["obs_feat"][e], S["ref_kf"][m], S["ref_feat"][m], what=R.NORMAL_DEPTH, fetch=fetch)
    return new


# ---------------------------------------------------------------------------------------------------------------- 1. SIM3
@pytest.mark.parametrize("in_order", (False, True))
def test_sim3_both_orders(ctx, world, in_order):
    Cs, rows, kfs = world
    S = Cs["S"]; owner = Cs["owner"]; before = _before(Cs, rows)
    _reset(kfs, S)
    with _table(ctx, rows) as t:
        out = _correct(t, Cs, kfs, in_order=in_order)
        # positions: the array route narrowed, bit for bit; numpy within its float64 bound plus one narrowing
        arr = Optimizer.CorrectMapPoints(before["pos"].astype("f8"), owner, Cs["sim3_before"], Cs["sim3_after"], ctx=ctx)
        assert out["pos"].tobytes() == arr.astype("f4").tobytes()
        ref = MC.sim3_positions(before["pos"], owner, Cs["sim3_before"], Cs["sim3_after"])
        exact = MC.correct_map_points_ref(before["pos"].astype("f8"), owner, Cs["sim3_before"], Cs["sim3_after"])
        err = np.abs(out["pos"].astype("f8") - exact)
        bound = 1e-12 + np.spacing(np.abs(exact).astype("f4")).astype("f8") / 2       # 1e-12 of the array route, half an ulp of the narrowing
        print("in_order=%s: max |pos - numpy| = %.3g, %d of %d rows differ from numpy narrowed" %
              (in_order, err.max(), (out["pos"] != ref).any(1).sum(), len(ref)))
        assert (err <= bound).all()
        moved = owner >= 0
        assert (out["pos"][moved] != before["pos"][moved]).any(1).all() and out["pos"][~moved].tobytes() == before["pos"][~moved].tobytes()
        # normal and depth: the restatement fed the device's own positions
        want = MC.correct(Cs, before, MC.SIM3, MC.IN_ORDER if in_order else MC.POSES_FIRST, pos_after=out["pos"])
        for k in OUT:
            assert _same_floats(out[k], want[k]), k
        keep = ~moved | (S["counts"] == 0)
        assert keep.sum() >= 50 and (moved & (S["counts"] == 0)).sum() >= 5
        for k in ("normal", "min_dist", "max_dist"):
            assert out[k][keep].tobytes() == before[k][keep].tobytes(), k
        other = MC.correct(Cs, before, MC.SIM3, MC.POSES_FIRST if in_order else MC.IN_ORDER, pos_after=out["pos"])
        many = moved & (S["counts"] >= 2)                         # the rule is visible (test_map_correct_cpu.py::test_scene_conditions)
        assert (out["normal"].view("u4") != other["normal"].view("u4")).any(1)[many].sum() > 0.5 * many.sum()
        _check_table(t, Cs, rows, out)
        _check_poses(kfs, Cs, *_sim3_poses(Cs))
        assert np.array(_sim3_poses(Cs)[0]).tobytes() == want["Tcw"].tobytes() and np.array(_sim3_poses(Cs)[1]).tobytes() == want["Ow"].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 2. old route
def test_poses_first_equals_todays_route(ctx, world):
    Cs, rows, kfs = world
    S = Cs["S"]
    _reset(kfs, S)
    with _table(ctx, rows) as t:
        _old_route(ctx, t, Cs, kfs)
        old = t.fetch(np.arange(R.CAPACITY))
        old_poses = [h.pose() for h in kfs]
    _reset(kfs, S)
    with _table(ctx, rows) as t:
        out = _correct(t, Cs, kfs)
        new = t.fetch(np.arange(R.CAPACITY))
        new_poses = [h.pose() for h in kfs]
    for k in COLS + ("seen",):
        assert old[k].tobytes() == new[k].tobytes(), k
    for (Ta, Oa), (Tb, Ob) in zip(old_poses, new_poses):
        assert Ta.tobytes() == Tb.tobytes() and Oa.tobytes() == Ob.tobytes()
    for k in OUT:
        assert out[k].tobytes() == new[k][S["slot"]].tobytes(), k


# ---------------------------------------------------------------------------------------------------------------- 3. RIGID
def test_rigid(ctx, world):
    Cs, rows, kfs = world
    S = Cs["S"]; before = _before(Cs, rows)
    _reset(kfs, S)
    want = MC.correct(Cs, before, MC.RIGID, lists=False)
    assert (want["pos"][Cs["owner"] >= 0] != before["pos"][Cs["owner"] >= 0]).any(1).all()
    with _table(ctx, rows) as t:
        out = _correct(t, Cs, kfs, rigid=True, with_lists=False)
        for k in OUT:
            assert out[k].tobytes() == want[k].tobytes(), k
        assert out["normal"].tobytes() == before["normal"].tobytes()
        _check_table(t, Cs, rows, want)
        _check_poses(kfs, Cs, Cs["Tcw_after"].reshape(-1, 3, 4), Cs["Ow_after"])
    _reset(kfs, S)                                                # with lists: normal and depth from the rigid positions
    want = MC.correct(Cs, before, MC.RIGID, MC.IN_ORDER)
    with _table(ctx, rows) as t:
        out = _correct(t, Cs, kfs, rigid=True, in_order=True)
        for k in OUT:
            assert _same_floats(out[k], want[k]), k
        _check_table(t, Cs, rows, want)


# ---------------------------------------------------------------------------------------------------------------- 4. sizes
@pytest.mark.parametrize("n_points", (0, 1, 3, 4, 5, 255, 256, 257))
def test_sizes(ctx, world, n_points):
    Cs, rows, kfs = world
    S = Cs["S"]
    sel = np.arange(n_points)
    if n_points == 1:
        sel = np.flatnonzero((S["counts"] == 65) & (Cs["owner"] >= 0))[:1]      # one point, more than one batch of observations
    before = {k: rows[k][S["slot"][sel]] for k in COLS}
    sub = dict(Cs, S=dict(S, slot=S["slot"][sel], counts=S["counts"][sel], ref_kf=S["ref_kf"][sel], ref_feat=S["ref_feat"][sel],
                          obs_first=np.concatenate([[0], np.cumsum(S["counts"][sel])]).astype("i4"),
                          obs_kf=np.concatenate([S["obs_kf"][S["obs_first"][p]:S["obs_first"][p + 1]] for p in sel] + [np.zeros(0, "i4")]),
                          obs_feat=np.concatenate([S["obs_feat"][S["obs_first"][p]:S["obs_first"][p + 1]] for p in sel] + [np.zeros(0, "i4")])))
    cases = [(Cs["n_moved"], Cs["owner"][sel]), (len(kfs), Cs["owner"][sel]), (1, np.where(Cs["owner"][sel] >= 0, 0, -1).astype("i4")),
             (Cs["n_moved"], np.full(n_points, Cs["n_moved"] - 1, "i4")), (Cs["n_moved"], np.full(n_points, -1, "i4"))]
    for nm, owner in cases:
        C2 = sub
        if nm > Cs["n_moved"]:                                    # every keyframe moves: three more Sim3 pairs
            extra = MC.scene(2)
            C2 = dict(sub, sim3_before=np.concatenate([Cs["sim3_before"], extra["sim3_before"][:3]]),
                      sim3_after=np.concatenate([Cs["sim3_after"], extra["sim3_after"][:3]]))
        _reset(kfs, S)
        with _table(ctx, rows) as t:
            out = t.correct(kfs, nm, S["slot"][sel], owner, sim3_before=C2["sim3_before"][:nm], sim3_after=C2["sim3_after"][:nm], in_order=True,
                            lists=MC.lists(sub["S"]))
            arr = Optimizer.CorrectMapPoints(before["pos"].astype("f8"), owner, C2["sim3_before"][:nm], C2["sim3_after"][:nm], ctx=ctx) if n_points else \
                np.zeros((0, 3))
            assert out["pos"].tobytes() == arr.astype("f4").tobytes()
            want = MC.correct(C2, before, MC.SIM3, MC.IN_ORDER, pos_after=out["pos"], n_moved=nm, owner=owner)
            for k in OUT:
                assert _same_floats(out[k], want[k]), (k, nm)
            if (owner < 0).all():
                for k in OUT:
                    assert out[k].tobytes() == before[k].tobytes(), k
            _check_table(t, sub, rows, want)
            _check_poses(kfs, Cs, want["Tcw"], want["Ow"])        # the poses are published whatever the points


# ---------------------------------------------------------------------------------------------------------------- 5. no sync
def test_form_without_outputs_and_search_local_points_afterwards(ctx, world):
    Cs, rows, kfs = world
    S = Cs["S"]; before = _before(Cs, rows)
    want = MC.correct(Cs, before, MC.SIM3, MC.POSES_FIRST)
    T, Ow = SLP.camera(rotvec=(0.03, -0.05, 0.02), t=(0.0, 0.0, 4.0))
    ok = (S["counts"] > 0) & (Cs["owner"] >= 0) & ~np.isnan(want["normal"]).any(1)
    sub = np.flatnonzero(ok)[:200]
    fr = SLP.frustum(want["pos"][sub], want["normal"][sub], want["min_dist"][sub], want["max_dist"][sub], T, Ow)
    vis = fr["gate"] == 0
    assert vis.sum() >= 50
    view = FrameGridView(fr["u"][vis], fr["v"][vis], fr["level"][vis], before["desc"][sub][vis])
    res = []
    for one_call in (True, False):
        _reset(kfs, S)
        with _table(ctx, rows) as t, DeviceFrame(view, None, ctx=ctx) as f:
            if one_call:
                assert _correct(t, Cs, kfs, fetch=False) is None
            else:
                _old_route(ctx, t, Cs, kfs, fetch=False)
            res.append(Tracking.SearchLocalPoints(f, t, T, SLP.INTR, SLP.SCALE, Ow=Ow, log_scale_factor=SLP.LOG_SF, taps=True))
            if one_call:
                got = t.fetch(S["slot"])
                arr = Optimizer.CorrectMapPoints(before["pos"].astype("f8"), Cs["owner"], Cs["sim3_before"], Cs["sim3_after"], ctx=ctx)
                assert got["pos"].tobytes() == arr.astype("f4").tobytes()
    a, b = res
    assert a["nmatches"] == b["nmatches"] and a["n_to_match"] == b["n_to_match"] >= 50 and a["nmatches"] >= 1
    for k in ("match", "mp_id", "in_view_slot", "level", "occupied", "proj_x", "proj_y", "view_cos"):
        assert a[k].tobytes() == b[k].tobytes(), k
    print("downstream: %d in view, %d matches" % (a["n_to_match"], a["nmatches"]))


# ---------------------------------------------------------------------------------------------------------------- 6. view
def test_through_a_view_on_a_second_context(ctx, world):
    Cs, rows, kfs = world
    S = Cs["S"]
    _reset(kfs, S)
    with _table(ctx, rows) as t:
        alone = _correct(t, Cs, kfs, in_order=True)
    other = _lib.Context(0)
    try:
        kfs_b = [_handle(other, kf) for kf in S["kfs"]]
        with _table(ctx, rows) as root, root.attach(other) as view:
            out = _correct(view, Cs, kfs_b, in_order=True, fetch=False)
            assert out is None
            got = root.fetch(S["slot"])                           # through the root table, in its own context
            for k in OUT:
                assert _same_floats(got[k], alone[k]), k
            _check_table(root, Cs, rows, alone)
            _check_poses(kfs_b, Cs, *_sim3_poses(Cs))
        for h in kfs_b:
            h.close()
    finally:
        other.close()


# ---------------------------------------------------------------------------------------------------------------- 7. errors
def _raw(ctx, t, kfl, n_moved, slot, owner, first, okf, ofeat, rkf, rfeat, outs, transform=0, order=0, sb=None, sa=None, Ta=None, Oa=None):
    a = lambda v, d="i4": None if v is None else np.ascontiguousarray(v, d)  # noqa: E731
    slot, owner, first, okf, ofeat, rkf, rfeat = [a(v) for v in (slot, owner, first, okf, ofeat, rkf, rfeat)]
    sb, sa, Ta, Oa = a(sb, "f8"), a(sa, "f8"), a(Ta, "f4"), a(Oa, "f4")
    handles = (C.c_void_p * max(len(kfl), 1))(*[k.handle for k in kfl])
    u = _lib.MapCorrect(len(kfl), handles, n_moved, transform, order, _lib.ptr(sb), _lib.ptr(sa), _lib.ptr(Ta), _lib.ptr(Oa), len(slot),
                        _lib.ptr(slot), _lib.ptr(owner), _lib.ptr(first), _lib.ptr(okf), _lib.ptr(ofeat), _lib.ptr(rkf), _lib.ptr(rfeat),
                        *[_lib.ptr(outs[k]) for k in OUT])
    return ctx.lib.ccm_map_table_correct_frames(ctx.handle, C.c_void_p(t.handle), C.byref(u))


def test_errors_leave_table_handles_and_outputs_untouched(ctx, world):
    Cs, rows, kfs = world
    S = Cs["S"]
    kf0 = S["kfs"][0]
    _reset(kfs, S)
    sb, sa = Cs["sim3_before"][:2], Cs["sim3_after"][:2]
    # three keyframes, two of them moved; two points: the first sees features 5 and 6 of kfs[0] and 7 of kfs[2], the second 8 of kfs[1]
    good = dict(n_moved=2, slot=[3, 9], owner=[1, 0], first=[0, 3, 4], okf=[0, 0, 2, 1], ofeat=[5, 6, 7, 8], rkf=[0, 1], rfeat=[5, 8], sb=sb, sa=sa)
    rigid = dict(good, transform=1, sb=None, sa=None, Ta=Cs["Tcw_after"][:2], Oa=Cs["Ow_after"][:2])
    other = _lib.Context(0)
    try:
        with _table(ctx, rows) as t, _handle(ctx, kf0, pose=False) as no_pose, _handle(ctx, kf0, camera=False) as no_cam, \
                _handle(other, kf0) as foreign, MapPointTable(16, ctx=other) as foreign_table:
            def outs():
                return dict(pos=np.full((2, 3), 77, "f4"), normal=np.full((2, 3), 77, "f4"), min_dist=np.full(2, 77, "f4"), max_dist=np.full(2, 77, "f4"))

            def refused(code, base=good, kfl=None, tab=None, **change):
                o = outs()
                kfl_ = kfs[:3] if kfl is None else kfl
                rc = _raw(ctx, t if tab is None else tab, kfl_, outs=o, **dict(base, **change))
                assert rc == code, (rc, change, ctx.lib.ccm_last_error(ctx.handle))
                assert all((v == 77).all() for v in o.values())
                got = t.fetch(np.arange(R.CAPACITY))
                for k in COLS:
                    assert (got[k].view(np.uint8) == rows[k].view(np.uint8)).all(), k
                _check_poses(kfs, Cs, [], [])
                return ctx.lib.ccm_last_error(ctx.handle)
            refused(E_ARG, sb=None)                               # a NULL required array for the chosen transform
            refused(E_ARG, sa=None)
            refused(E_ARG, base=rigid, Ta=None)
            refused(E_ARG, base=rigid, Oa=None)
            refused(E_ARG, owner=None)
            refused(E_ARG, rkf=None)                              # with obs_first the reference lists are required
            refused(E_ARG, okf=None)
            refused(E_ARG, transform=2)
            refused(E_ARG, order=2)
            refused(E_ARG, order=-1)
            refused(E_ARG, n_moved=4)                             # n_moved outside [0, n_kf]
            refused(E_ARG, n_moved=-1)
            refused(E_ARG, kfl=[kfs[0], kfs[1], kfs[0]])          # a handle twice
            refused(E_ARG, slot=[3, R.CAPACITY])                  # a slot out of range
            refused(E_ARG, slot=[3, -1])
            refused(E_ARG, slot=[3, 3])                           # a slot twice
            refused(E_ARG, owner=[1, 2])                          # owner >= n_moved
            bad = sa.copy(); bad[1, 5] = np.nan
            refused(E_ARG, sa=bad)
            bad = sb.copy(); bad[0, 0] = np.inf
            refused(E_ARG, sb=bad)
            bad = sa.copy(); bad[0, 7] = 0.0
            refused(E_ARG, sa=bad)                                # s <= 0 in sim3_after
            bad = sa.copy(); bad[1, 7] = -1.0
            refused(E_ARG, sa=bad)
            refused(E_ARG, first=[0, 3, 2])                       # the list errors of ccm_map_refresh
            refused(E_ARG, first=[1, 3, 4])
            refused(E_ARG, okf=[0, 0, 3, 1])
            msg = refused(E_ARG, ofeat=[5, 300, 7, 8])
            assert b"point 0" in msg and b"entry 1" in msg
            refused(E_ARG, rkf=[0, 3])
            refused(E_ARG, rfeat=[300, 8])
            refused(E_ARG, kfl=[kfs[0], kfs[1], foreign])         # a handle of a second context
            refused(E_ARG, tab=foreign_table)                     # a table of a second context
            msg = refused(E_STATE, kfl=[kfs[0], kfs[1], no_pose]) # an observed handle without a pose
            assert b"pose" in msg
            msg = refused(E_STATE, kfl=[kfs[0], kfs[1], no_cam], rkf=[2, 1], rfeat=[7, 8])    # a reference handle without a camera
            assert b"camera" in msg
            msg = refused(E_STATE, base=rigid, kfl=[kfs[0], no_pose, kfs[2]], first=None, okf=None, ofeat=None, rkf=None, rfeat=None)
            assert b"pose" in msg                                 # RIGID: an owner handle without a pose
            o = outs()                                            # n_moved == 0 with no points is OK and touches nothing
            assert _raw(ctx, t, kfs[:3], 0, [], [], None, None, None, None, None, o) == 0 and all((v == 77).all() for v in o.values())
        orphan = MapPointTable(16, ctx=other)
        orphan_kf = _handle(other, kf0)
    finally:
        other.close()
    o = dict(pos=np.full((2, 3), 77, "f4"), normal=np.full((2, 3), 77, "f4"), min_dist=np.full(2, 77, "f4"), max_dist=np.full(2, 77, "f4"))
    assert _raw(ctx, orphan, kfs[:3], outs=o, **good) == E_STATE   # a table that outlived its context
    with _table(ctx, rows) as t:
        assert _raw(ctx, t, [kfs[0], kfs[1], orphan_kf], outs=o, **good) == E_STATE   # and a handle that did
        got = t.fetch(np.arange(R.CAPACITY))
        for k in COLS:
            assert (got[k].view(np.uint8) == rows[k].view(np.uint8)).all(), k
    assert all((v == 77).all() for v in o.values())
    _check_poses(kfs, Cs, [], [])
    orphan.close(); orphan_kf.close()


# ---------------------------------------------------------------------------------------------------------------- 8. repeat
def test_repeated_call_on_restored_rows_gives_identical_bytes(ctx, world):
    Cs, rows, kfs = world
    S = Cs["S"]
    res = []
    with _table(ctx, rows) as t:
        for _ in range(2):
            _reset(kfs, S)
            t.update(np.arange(R.CAPACITY), **{k: rows[k] for k in COLS})
            out = _correct(t, Cs, kfs, in_order=True)
            res.append((out, t.fetch(np.arange(R.CAPACITY)), [h.pose() for h in kfs]))
            t.fetch(np.arange(7))                                 # another user of the context's staging in between
    (a, ta, pa), (b, tb, pb) = res
    for k in OUT:
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in COLS:
        assert ta[k].tobytes() == tb[k].tobytes(), k
    for (Ta, Oa), (Tb, Ob) in zip(pa, pb):
        assert Ta.tobytes() == Tb.tobytes() and Oa.tobytes() == Ob.tobytes()
