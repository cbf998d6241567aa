"""Frame handles: ccm_frame_compute_bow, ccm_frame_search_by_bow and ccm_search_by_bow_frames (Tracking::TrackReferenceKeyFrame,
src/Tracking.cpp:514-556, and the SearchByBoW loop in front of the batched Sim3Solver).

Everything is compared for equality of integers or bytes: the transform and the matcher with the CPU oracle, the node directory with
its numpy restatement and with ccm_frame_set_bow, the handle calls with the array calls (ccm_match_bow, ccm_pose_optimize) of the
same library.  The pose of the chain must be bit-equal to the array chain's: the same kernel gets the same problem.  The synthetic
vocabulary and frames come from tests/frame_bow_ref.py."""
import ctypes as C

import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher
from motioncheck_ccm_slam_amd.optimizer import Optimizer
from motioncheck_ccm_slam_amd.tracking import Tracking
from motioncheck_ccm_slam_amd.vocabulary import ORBVocabulary
import create_new_map_points_ref as ref
import frame_bow_ref as fb
from keyframe_handles_ref import directory
from test_keyframe_handles_gpu import _close, _frames, _ids, _same

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -7
DIR_MAX = 4096                                   # frames above it get their directory from the host build
LU = 3                                           # node level 1 of the 4-level tree: about a hundred features per node


@pytest.fixture(scope="module")
def tr():
    return fb.tree()


@pytest.fixture(scope="module")
def voc(ctx, tr):
    return ORBVocabulary(fb.K, fb.L, *tr, ctx=ctx)


@pytest.fixture(scope="module")
def rvoc(oracle, tr):
    return oracle.Voc(fb.K, fb.L, *tr)


@pytest.fixture(scope="module")
def world(tr, rvoc):
    """One reference keyframe and four frames that see it again, with the oracle's nodes at LU and at level 2"""
    kf = fb.make_kf(tr, 3, 700)
    views = [fb.make_view(tr, kf, 1, 900), fb.make_view(tr, kf, 2, 500), fb.make_view(tr, kf, 5, 1000, share=0.3), fb.make_view(tr, kf, 6, 300)]
    for d in [kf] + views:
        d["node"] = fb.expected_node(rvoc, d["desc"], LU)[2]
        d["node2"] = fb.expected_node(rvoc, d["desc"], 2)[2]
    return kf, views


def _frame(ctx, d, angle=True, ids=None):
    f = DeviceFrame(FrameGridView(d["kx"], d["ky"], d["oct"], d["desc"]), d["angle"] if angle else None, ctx=ctx)
    if ids is not None:
        f.map_points = ids
    return f


def _plain(rng, desc):
    n = len(desc)
    kx, ky, octv = fb.keypoints(rng, n)
    return dict(kx=kx, ky=ky, oct=octv, desc=desc, angle=rng.uniform(0, 360, n).astype("f4"))


def _same_dir(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()


def _orphan(d):
    """A handle whose context is gone"""
    other = _lib.Context(0)
    f = _frame(other, d)
    other.close()
    return f


# ------------------------------------------------------------------------------------------------------------ 1. compute_bow
def _check_compute_bow(ctx, voc, rvoc, feats, levelsup):
    rng = np.random.default_rng(len(feats))
    wid, w, node = fb.expected_node(rvoc, feats, levelsup)
    d = _plain(rng, feats)
    with _frame(ctx, d) as f, _frame(ctx, d) as g, _frame(ctx, d) as q:
        got = f.compute_bow(voc, levelsup)
        assert (got[0] == wid).all() and (got[1] == w).all() and (got[2] == node).all()
        want = directory(node)
        _same_dir(f.bow(), want)
        g.set_bow(node)
        _same_dir(f.bow(), g.bow())
        assert q.compute_bow(voc, levelsup, outputs=False) is None       # the form that reads back two counters only
        _same_dir(q.bow(), want)
    return node


def test_compute_bow_matches_oracle_and_set_bow(ctx, tr, voc, rvoc):
    rng = np.random.default_rng(0)
    seen_stopped = seen_big = False
    for n in (0, 1, 63, 64, 65, 1000, DIR_MAX, DIR_MAX + 1):
        feats = fb.features(tr, rng, n)
        for levelsup in (0, LU, fb.L):
            node = _check_compute_bow(ctx, voc, rvoc, feats, levelsup)
            if n == 1000 and levelsup == LU:
                seen_stopped = bool((node < 0).any())
                seen_big = bool(np.bincount(node[node >= 0]).max() > 64)
    assert seen_stopped and seen_big                                    # else the cases above show nothing
    stopped, live = fb.words(tr)
    par, desc, w = tr
    one = _check_compute_bow(ctx, voc, rvoc, np.repeat(desc[live[3]][None], 130, 0), 2)
    assert len(np.unique(one)) == 1 and one[0] >= 0                     # all features in one node
    none = _check_compute_bow(ctx, voc, rvoc, desc[stopped[rng.integers(0, len(stopped), 130)]], 2)
    assert (none == -1).all()                                           # every feature a stopped word


def test_compute_bow_with_an_empty_vocabulary(ctx, oracle):
    z = np.zeros((1, 32), np.uint8)
    empty = ORBVocabulary(10, 6, [0], z, [0.0], ctx=ctx)
    rempty = oracle.Voc(10, 6, [0], z, [0.0])
    feats = np.random.default_rng(1).integers(0, 256, (65, 32), dtype=np.uint8)
    node = _check_compute_bow(ctx, empty, rempty, feats, 4)
    assert (node == -1).all() and empty.size() == 0


def test_compute_bow_replaces_an_earlier_bow(ctx, tr, voc, rvoc):
    rng = np.random.default_rng(2)
    feats = fb.features(tr, rng, 500)
    with _frame(ctx, _plain(rng, feats)) as f:
        f.set_bow(rng.integers(-1, 50, 500))
        for levelsup in (2, LU, 2):
            f.compute_bow(voc, levelsup, outputs=False)
            _same_dir(f.bow(), directory(fb.expected_node(rvoc, feats, levelsup)[2]))


def test_computed_bow_serves_create_new_map_points(ctx, voc, rvoc):
    """A handle with camera, pose and a computed bow gives ccm_create_new_map_points_frames the bytes set_bow gives, setters in both orders"""
    sc = ref.make_small(ref.make_scene(), 64, (3, 8, 9))
    sc["epipole"] = np.array([ref.epipole32(sc["current"], kf) for kf in sc["neighbours"]], "f4").reshape(-1, 2)
    kfs = [sc["current"]] + list(sc["neighbours"])
    nodes = [fb.expected_node(rvoc, d["desc"], LU)[2] for d in kfs]
    assert any((nd < 0).any() for nd in nodes) and max(len(d["desc"]) for d in kfs) > 3000

    def handle(d, node, order):
        f = DeviceFrame(FrameGridView(d["kp_x"], d["kp_y"], d["kp_octave"], d["desc"]), ctx=ctx)
        f.map_points = _ids(d["has_mp"])
        for step in order:
            if step == "c":
                f.set_camera(d["K"], d["scale_factors"], d["level_sigma2"])
            elif step == "b":
                f.set_bow(node)
            elif step == "B":
                f.compute_bow(voc, LU, outputs=False)
            elif step == "p":
                f.set_pose(d["Tcw"], d["Ow"])
        return f

    hs = [handle(d, nd, "cbp") for d, nd in zip(kfs, nodes)]
    want = _frames(ctx, hs[0], hs[1:], sc)
    _close(hs[0], hs[1:])
    assert want["n_new"] > 0
    for order in ("cBp", "pBc"):
        hs = [handle(d, nd, order) for d, nd in zip(kfs, nodes)]
        _same(_frames(ctx, hs[0], hs[1:], sc), want)
        _close(hs[0], hs[1:])


def test_compute_bow_errors(ctx, tr, voc):
    rng = np.random.default_rng(3)
    d = _plain(rng, fb.features(tr, rng, 200))
    lib = ctx.lib; p = _lib.ptr
    other = _lib.Context(0)
    try:
        alien_voc = ORBVocabulary(fb.K, fb.L, *tr, ctx=other)
        with _frame(ctx, d) as f, _frame(other, d) as alien:
            f.set_bow(rng.integers(-1, 30, 200))
            before = f.bow()
            wid = np.full(200, 7, "i4"); w = np.full(200, 7.0); node = np.full(200, 7, "i4")

            def call(c, fr, v, *out):
                return lib.ccm_frame_compute_bow(c.handle, C.c_void_p(fr.handle), v.handle, LU, *out)
            assert call(ctx, f, alien_voc, p(wid), p(w), p(node)) == E_ARG        # a vocabulary of another context
            assert call(ctx, alien, voc, p(wid), p(w), p(node)) == E_ARG          # a handle of another context
            assert call(ctx, f, voc, p(wid), None, p(node)) == E_ARG              # all three outputs or none
            assert (wid == 7).all() and (w == 7).all() and (node == 7).all()
            _same_dir(f.bow(), before)                                            # the previous bow is intact
        del alien_voc
    finally:
        other.close()
    gone = _orphan(d)
    assert lib.ccm_frame_compute_bow(ctx.handle, C.c_void_p(gone.handle), voc.handle, LU, None, None, None) == E_STATE
    gone.close()


# ------------------------------------------------------------------------------------------------------------ 2. search_by_bow
def _search_case(ctx, oracle, kfh, fh, kf, f, node1, node2, nnratio, ori, valid1):
    """One SearchByBoW(KeyFrame, Frame) on handles against ccm_match_bow and the oracle; -> the oracle's count"""
    m = ORBmatcher(nnratio, ori, ctx=ctx)
    n2 = len(f["desc"])
    v1 = (kf["ids"] >= 0).astype(np.uint8) if valid1 is None else valid1
    rn, r12 = oracle.match_bow(nnratio, ori, 50, False, kf["desc"], node1, v1, kf["angle"], f["desc"], node2, None, f["angle"])
    an, a12 = m.SearchByBoW(kf["desc"], node1, v1, kf["angle"], f["desc"], node2, f["angle"])
    assert an == rn and (a12 == r12).all()
    want = fb.invert(r12, n2)
    mark = (np.arange(n2) + 5).astype("i4")
    fh.map_points = mark
    n, match = m.SearchByBoWHandle(kfh, fh, valid1, min_matches=rn + 1)
    assert n == rn and (match == want).all()
    assert (fh.map_points == mark).all()                                # too few matches: mp_id untouched
    n, match = m.SearchByBoWHandle(kfh, fh, valid1, min_matches=rn)
    assert n == rn and (match == want).all()
    assert (fh.map_points == np.where(want >= 0, kf["ids"][np.maximum(want, 0)], -1)).all()   # replaced as a whole
    return rn


def test_search_by_bow_matches_match_bow_and_oracle(ctx, oracle, world, voc):
    kf, views = world
    rng = np.random.default_rng(4)
    given = (rng.random(len(kf["desc"])) < 0.7).astype(np.uint8)
    for f in (views[0], views[3]):
        c1 = np.bincount(kf["node"][kf["node"] >= 0], minlength=6000); c2 = np.bincount(f["node"][f["node"] >= 0], minlength=6000)
        with _frame(ctx, kf, ids=kf["ids"]) as kfh, _frame(ctx, f) as fh:
            assert (kfh.compute_bow(voc, LU)[2] == kf["node"]).all() and (fh.compute_bow(voc, LU)[2] == f["node"]).all()
            for nnratio in (0.7, 0.9):
                for valid1 in (None, given):
                    plain = _search_case(ctx, oracle, kfh, fh, kf, f, kf["node"], f["node"], nnratio, False, valid1)
                    turned = _search_case(ctx, oracle, kfh, fh, kf, f, kf["node"], f["node"], nnratio, True, valid1)
                    assert turned > 0 and plain > turned                # the rotation filter removed at least one match
        if f is views[0]:
            assert ((c1 > 64) & (c2 > 64)).any()                        # a common node past the lane stride on both sides


def test_search_by_bow_shapes(ctx, oracle, world, voc, tr):
    kf, views = world
    f = views[1]
    with _frame(ctx, kf, ids=kf["ids"]) as kfh, _frame(ctx, f) as fh:
        kfh.set_bow(kf["node"])                                         # set_bow on one side, compute_bow on the other
        fh.compute_bow(voc, LU, outputs=False)
        assert _search_case(ctx, oracle, kfh, fh, kf, f, kf["node"], f["node"], 0.7, True, None) > 0
        # no common node
        far = np.where(f["node"] >= 0, f["node"] + 100000, -1).astype("i4")
        fh.set_bow(far)
        assert _search_case(ctx, oracle, kfh, fh, kf, f, kf["node"], far, 0.7, True, None) == 0
        # a keyframe with no valid point: as a mask, and as mp_id all -1
        fh.set_bow(f["node"])
        none = np.zeros(len(kf["desc"]), np.uint8)
        assert _search_case(ctx, oracle, kfh, fh, kf, f, kf["node"], f["node"], 0.7, True, none) == 0
        kfh.map_points = None
        n, match = ORBmatcher(0.7, True, ctx=ctx).SearchByBoWHandle(kfh, fh, None, min_matches=1)
        assert n == 0 and (match == -1).all()
        kfh.map_points = kf["ids"]
        # an empty frame, and an empty keyframe
        e = {k: v[:0] for k, v in f.items()}
        with _frame(ctx, e) as eh:
            eh.compute_bow(voc, LU, outputs=False)
            n, match = ORBmatcher(0.7, True, ctx=ctx).SearchByBoWHandle(kfh, eh, None, min_matches=0)
            assert n == 0 and match.shape == (0,)
            mark = (np.arange(len(f["desc"])) + 5).astype("i4")
            fh.map_points = mark
            n, match = ORBmatcher(0.7, True, ctx=ctx).SearchByBoWHandle(eh, fh, None, min_matches=1)
            assert n == 0 and (match == -1).all() and (fh.map_points == mark).all()
            n, match = ORBmatcher(0.7, True, ctx=ctx).SearchByBoWHandle(eh, fh, None, min_matches=0)
            assert n == 0 and (fh.map_points == -1).all()              # 0 >= 0: replaced as a whole


# ------------------------------------------------------------------------------------------------------------ 3. the chain
def _array_chain(ctx, voc, kf, f, levelsup, nnratio=0.7):
    """TrackReferenceKeyFrame through host arrays: ccm_voc_transform + ccm_bow_vector, ccm_match_bow, ccm_pose_optimize"""
    _, _, fv = voc.transform(f["desc"], levelsup)
    v1 = (kf["ids"] >= 0).astype(np.uint8)
    nm, m12 = ORBmatcher(nnratio, True, ctx=ctx).SearchByBoW(kf["desc"], kf["node2"], v1, kf["angle"], f["desc"], fv, f["angle"])
    match = fb.invert(m12, len(fv))
    ids = np.where(match >= 0, kf["ids"][np.maximum(match, 0)], -1).astype("i4")
    has = ids >= 0
    pose, o, n = Optimizer.PoseOptimizationClient(fb.POSE0[None], fb.INTR[None], np.array([0, has.sum()], "i4"), kf["xyz"][ids[has]],
                                                  np.stack([f["kx"][has], f["ky"][has]], 1).astype("f8"),
                                                  fb.INV_SIGMA2[f["oct"][has]].astype("f8"), ctx=ctx)
    outl = np.zeros(len(ids), np.uint8); outl[has] = o
    ids[outl != 0] = -1
    return dict(nmatches=nm, match=match, pose=pose[0], outlier=outl, n_inliers=int(n[0]), mp_id=ids, nmatches_map=int((ids >= 0).sum()))


def test_track_reference_keyframe_equals_the_array_chain(ctx, world, voc):
    kf, views = world
    f = views[0]
    want = _array_chain(ctx, voc, kf, f, 2)
    assert want["nmatches"] >= 15 and want["outlier"].sum() > 0 and want["nmatches_map"] >= 10
    with _frame(ctx, kf, ids=kf["ids"]) as kfh, _frame(ctx, f) as fh:
        kfh.compute_bow(voc, 2, outputs=False)
        got = Tracking.TrackReferenceKeyFrame(fh, kfh, voc, fb.POSE0, fb.INTR, kf["xyz"], fb.INV_SIGMA2, levelsup=2)
        assert got["ok"] and got["nmatches"] == want["nmatches"] and (got["match"] == want["match"]).all()
        assert got["pose"].tobytes() == want["pose"].tobytes()
        assert (got["outlier"] == want["outlier"]).all() and got["n_inliers"] == want["n_inliers"]
        assert got["nmatches_map"] == want["nmatches_map"]
        assert (got["mp_id"] == want["mp_id"]).all() and (fh.map_points == want["mp_id"]).all()
        # the early return of :526: the frame keeps its map points
        mark = (np.arange(fh.n) + 5).astype("i4")
        fh.map_points = mark
        early = Tracking.TrackReferenceKeyFrame(fh, kfh, voc, fb.POSE0, fb.INTR, kf["xyz"], fb.INV_SIGMA2, levelsup=2,
                                                min_matches=want["nmatches"] + 1)
        assert not early["ok"] and early["nmatches"] == want["nmatches"] and (fh.map_points == mark).all()


# ------------------------------------------------------------------------------------------------------------ 4. the batch
def test_search_by_bow_frames_equals_the_pairs(ctx, oracle, world, voc):
    kf, views = world
    far = dict(views[1]); far["node"] = np.where(views[1]["node"] >= 0, views[1]["node"] + 100000, -1).astype("i4")
    cands = [views[0], views[2], views[0], far, views[3]]               # one repeated, one without a common node
    rng = np.random.default_rng(6)
    v1 = (rng.random(len(kf["desc"])) < 0.7).astype(np.uint8)
    v2 = [(rng.random(len(c["desc"])) < 0.8).astype(np.uint8) for c in cands]
    with _frame(ctx, kf, ids=kf["ids"]) as kfh:
        kfh.compute_bow(voc, LU, outputs=False)
        made = {}
        for c in cands:
            if id(c) not in made:
                h = _frame(ctx, c, ids=c["ids"])
                if c is far:
                    h.set_bow(c["node"])
                else:
                    h.compute_bow(voc, LU, outputs=False)
                made[id(c)] = h
        hs = [made[id(c)] for c in cands]
        total = 0
        for nnratio, ori, masks in ((0.7, True, True), (0.9, False, True), (0.7, True, False)):
            m = ORBmatcher(nnratio, ori, ctx=ctx)
            a1 = v1 if masks else (kf["ids"] >= 0).astype(np.uint8)
            nm, m12 = m.SearchByBoWFrames(kfh, hs, v1 if masks else None, v2 if masks else None)
            assert nm.shape == (5,) and m12.shape == (5, len(kf["desc"]))
            for k, c in enumerate(cands):
                a2 = v2[k] if masks else (c["ids"] >= 0).astype(np.uint8)
                rn, r12 = oracle.match_bow(nnratio, ori, 50, True, kf["desc"], kf["node"], a1, kf["angle"], c["desc"], c["node"], a2, c["angle"])
                an, a12 = m.SearchByBoW(kf["desc"], kf["node"], a1, kf["angle"], c["desc"], c["node"], c["angle"], valid2=a2)
                assert an == rn and (a12 == r12).all()
                assert nm[k] == rn and (m12[k] == r12).all(), (nnratio, ori, masks, k)
                assert (rn == 0) == (c is far)
                total += rn
            if not masks:                                               # the repeated handle, under the same derived mask
                assert (m12[0] == m12[2]).all() and nm[0] == nm[2] > 0
        assert total > 1000
        nm, m12 = ORBmatcher(0.7, True, ctx=ctx).SearchByBoWFrames(kfh, [])
        assert nm.shape == (0,) and m12.shape == (0, len(kf["desc"]))
        for h in made.values():
            h.close()


# ------------------------------------------------------------------------------------------------------------ 5. errors
def test_search_by_bow_errors_leave_everything_untouched(ctx, world, voc):
    kf, views = world
    f = views[3]
    lib = ctx.lib; p = _lib.ptr
    n1, n2 = len(kf["desc"]), len(f["desc"])
    mark = (np.arange(n2) + 5).astype("i4")
    other = _lib.Context(0)
    gone = _orphan(f)
    try:
        with _frame(ctx, kf, ids=kf["ids"]) as kfh, _frame(ctx, f, ids=mark) as fh, _frame(ctx, f, ids=mark) as nobow, \
                _frame(ctx, f, angle=False, ids=mark) as noang, _frame(other, f, ids=mark) as alien:
            kfh.compute_bow(voc, LU, outputs=False)
            for h in (fh, noang):
                h.compute_bow(voc, LU, outputs=False)
            alien.set_bow(f["node"])

            def single(c, a, b, ori=1):
                opt = _lib.BowOptions(0.7, ori, 50, 0)
                match = np.full(max(a.n, b.n), 7, "i4")
                rc = lib.ccm_frame_search_by_bow(c.handle, C.c_void_p(a.handle), C.c_void_p(b.handle), C.byref(opt), None, 0, p(match))
                return rc, bool((match == 7).all())

            def batch(c, a, bs, ori=1):
                opt = _lib.BowOptions(0.7, ori, 50, 1)
                m12 = np.full((len(bs), a.n), 7, "i4"); nm = np.full(len(bs), 7, "i4")
                arr = (C.c_void_p * len(bs))(*[b.handle for b in bs])
                rc = lib.ccm_search_by_bow_frames(c.handle, C.c_void_p(a.handle), len(bs), arr, C.byref(opt), None, None, None, p(m12), p(nm))
                return rc, bool((m12 == 7).all() and (nm == 7).all())

            for bad, code, ori in ((alien, E_ARG, 1), (nobow, E_STATE, 1), (noang, E_ARG, 1), (gone, E_STATE, 1)):
                assert single(ctx, kfh, bad, ori) == (code, True)
                assert batch(ctx, kfh, [fh, bad, fh], ori) == (code, True)
                if bad is not gone:
                    assert (bad.map_points == mark).all()
            assert single(ctx, nobow, fh) == (E_STATE, True) and batch(ctx, nobow, [fh]) == (E_STATE, True)
            assert single(other, kfh, fh)[0] == E_ARG                              # the handles of another context
            assert single(ctx, fh, fh) == (E_ARG, True)                            # one handle on both sides
            assert batch(ctx, kfh, [fh, nobow]) == (E_STATE, True) and "kfs2[1]" in lib.ccm_last_error(ctx.handle).decode()
            assert (fh.map_points == mark).all()
            rc, clean = single(ctx, kfh, noang, ori=0)                             # without the orientation check it runs
            assert rc > 0 and not clean
    finally:
        gone.close()
        other.close()


# ------------------------------------------------------------------------------------------------------------ 6. device memory
def test_no_device_memory_growth(ctx, world, voc):
    import torch
    kf, views = world
    free10 = None
    with _frame(ctx, kf, ids=kf["ids"]) as kfh:
        kfh.compute_bow(voc, 2, outputs=False)
        first = None
        for i in range(50):
            f = views[i % 4]
            with _frame(ctx, f, ids=f["ids"]) as fh:
                got = Tracking.TrackReferenceKeyFrame(fh, kfh, voc, fb.POSE0, fb.INTR, kf["xyz"], fb.INV_SIGMA2, levelsup=2)
                nm, _ = ORBmatcher(0.7, True, ctx=ctx).SearchByBoWFrames(kfh, [fh, fh])
            if i % 4 == 0:
                first = first or (got["nmatches"], int(nm[0]))
                assert (got["nmatches"], int(nm[0])) == first and nm[0] == nm[1]
            if i == 9:
                ctx.sync()
                free10 = torch.cuda.mem_get_info()[0]
    ctx.sync()
    assert torch.cuda.mem_get_info()[0] == free10
