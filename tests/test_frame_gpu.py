"""Frame handles (include/ccm_hot.h "frame handles") on the GPU: the device-built feature grid against a numpy restatement of
Frame::AssignFeaturesToGrid, the handle matchers and the handle pose against the host-buffer entry points and the CPU oracle, the
motion-model chain of Tracking on handles, misuse, the host-acceptance fallback and frame churn."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import optimizer_cases as C_
from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.matcher import FRAME_GRID_COLS, FRAME_GRID_ROWS, FrameGridView, ORBmatcher
from motioncheck_ccm_slam_amd.optimizer import Optimizer, pose_delta
from motioncheck_ccm_slam_amd.orb import ORBextractor

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -7


def _round_half_away(v):
    t = np.trunc(v)
    return t + np.sign(v) * (np.abs(v - t) >= np.float32(0.5))


def _np_grid(view: FrameGridView, cols=FRAME_GRID_COLS, rows=FRAME_GRID_ROWS):
    """Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cpp:103-118, 255-266) in float32: cell k = px*rows + py, index order."""
    fx = _round_half_away((view.kx - view.min_x) * view.inv_w)
    fy = _round_half_away((view.ky - view.min_y) * view.inv_h)
    ok = (fx >= 0) & (fx < cols) & (fy >= 0) & (fy < rows)
    cell = np.where(ok, fx.astype(np.int64) * rows + fy.astype(np.int64), -1)
    first = np.zeros(cols * rows + 1, "i4")
    np.add.at(first, cell[ok] + 1, 1)
    first = np.cumsum(first).astype("i4")
    idx = np.flatnonzero(ok)
    items = idx[np.argsort(cell[ok], kind="stable")].astype("i4")
    return first, items


def _extract(ctx, f=0, nfeat=1000, w=752, h=480):
    ex = ORBextractor(nfeat, 1.2, 8, 20, 7, ctx=ctx)
    kps, desc = ex(synth.frame(f, w, h))
    return ex, kps, desc


def _map_points(fr: FrameGridView, desc, seed, n_true=1200, n_rand=300):
    """Map points re-projected with noise from the frame's own features, plus unrelated ones (as tests/test_window_gpu.py)."""
    n = len(fr.kx)
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, n_true)
    flips = np.packbits(rng.random((n_true, 256)) < 0.05, axis=1, bitorder="little")
    nm = n_true + n_rand
    return dict(
        mp_desc=np.concatenate([desc[src] ^ flips, rng.integers(0, 256, (n_rand, 32), dtype=np.uint8)]),
        px=np.concatenate([fr.kx[src] + rng.normal(0, 1.5, n_true), rng.uniform(0, 752, n_rand)]).astype("f4"),
        py=np.concatenate([fr.ky[src] + rng.normal(0, 1.5, n_true), rng.uniform(0, 480, n_rand)]).astype("f4"),
        level=np.concatenate([np.clip(fr.oct[src] + rng.integers(0, 2, n_true), 0, 7), rng.integers(0, 8, n_rand)]).astype("i4"),
        view_cos=rng.uniform(0.99, 1.0, nm).astype("f4"), in_view=rng.random(nm) < 0.9, has_obs=rng.random(nm) < 0.95,
        occupied=rng.random(n) < 0.2)


def _sbp_both(m, fr, handle, sf, mp, th, qid=None):
    a = m.SearchByProjection(fr, sf, mp["in_view"], mp["level"], mp["view_cos"], mp["px"], mp["py"], mp["mp_desc"], mp["has_obs"],
                             mp["occupied"], th)
    b = m.SearchByProjectionHandle(handle, sf, mp["in_view"], mp["level"], mp["view_cos"], mp["px"], mp["py"], mp["mp_desc"],
                                   mp["has_obs"], mp["occupied"], th, query_mp_id=qid)
    return a, b


def _same(a, b):
    return a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all()


# ---------------------------------------------------------------------------------------------------------------- 1. grid
def test_grid_matches_assign_features_to_grid(ctx):
    ex, kps, desc = _extract(ctx, 0)
    fr = FrameGridView(kps["x"], kps["y"], kps["octave"], desc)
    with DeviceFrame.from_extract(ex, 0, ctx=ctx) as h:
        first, items = h.grid()
        rf, ri = _np_grid(fr)
        assert h.n == len(kps) and (first == rf).all() and (items == ri).all()
        assert (np.diff(rf) > 1).sum() > 20                       # cells with several features: the in-cell order is exercised
    # bounds that crop: features left of min_x / above min_y / beyond max_x drop out
    fr2 = FrameGridView(kps["x"], kps["y"], kps["octave"], desc, min_x=40.0, max_x=700.0, min_y=30.0, max_y=450.0)
    with DeviceFrame(fr2, kps["angle"], ctx=ctx) as h:
        first, items = h.grid()
        rf, ri = _np_grid(fr2)
        assert (first == rf).all() and (items == ri).all() and rf[-1] < len(kps)
    # N = 0
    z = FrameGridView(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 32)))
    with DeviceFrame(z, np.zeros(0), ctx=ctx) as h:
        first, items = h.grid()
        assert h.n == 0 and (first == 0).all() and len(items) == 0
        assert (h.map_points == np.zeros(0)).all()
    # 1920 x 1080, 3000 features
    ex3, k3, d3 = _extract(ctx, 1, 3000, 1920, 1080)
    assert len(k3) > 2000
    fr3 = FrameGridView(k3["x"], k3["y"], k3["octave"], d3, max_x=1920.0, max_y=1080.0)
    for h in (DeviceFrame(fr3, k3["angle"], ctx=ctx), DeviceFrame.from_extract(ex3, 0, max_x=1920.0, max_y=1080.0, ctx=ctx)):
        first, items = h.grid()
        rf, ri = _np_grid(fr3)
        assert (first == rf).all() and (items == ri).all()
        h.close()


# ---------------------------------------------------------------------------------------------------------------- 2. construction
def test_construction_paths_agree(ctx):
    ex, kps, desc = _extract(ctx, 1)
    sf = ex.GetScaleFactors()
    rng = np.random.default_rng(11)
    kxu = (kps["x"] + rng.normal(0, 0.7, len(kps))).astype("f4"); kyu = (kps["y"] + rng.normal(0, 0.7, len(kps))).astype("f4")
    m = ORBmatcher(0.8, ctx=ctx)
    for undist, (kx, ky) in ((False, (kps["x"], kps["y"])), (True, (kxu, kyu))):
        fr = FrameGridView(kx, ky, kps["octave"], desc)
        mp = _map_points(fr, desc, 2)
        ex(synth.frame(1))                                         # the extract the handle copies from
        hx = DeviceFrame.from_extract(ex, 0, kx if undist else None, ky if undist else None, ctx=ctx)
        hc = DeviceFrame(fr, kps["angle"], ctx=ctx)
        g1, g2, rf = hx.grid(), hc.grid(), _np_grid(fr)
        assert all((a == b).all() and (a == c).all() for a, b, c in zip(g1, g2, rf))
        ref = m.SearchByProjection(fr, sf, mp["in_view"], mp["level"], mp["view_cos"], mp["px"], mp["py"], mp["mp_desc"], mp["has_obs"],
                                   mp["occupied"], 3.0)
        for h in (hx, hc):
            got = m.SearchByProjectionHandle(h, sf, mp["in_view"], mp["level"], mp["view_cos"], mp["px"], mp["py"], mp["mp_desc"],
                                             mp["has_obs"], mp["occupied"], 3.0)
            assert _same(ref, got) and ref[0] > 300
        hx.close(); hc.close()


# ---------------------------------------------------------------------------------------------------------------- 3. SearchByProjection
@pytest.mark.parametrize("th", [1.0, 3.0])
def test_handle_search_by_projection(ctx, oracle, th):
    ex, kps, desc = _extract(ctx, 1)
    sf = ex.GetScaleFactors()
    fr = FrameGridView(kps["x"], kps["y"], kps["octave"], desc)
    mp = _map_points(fr, desc, 1)
    m = ORBmatcher(0.8, ctx=ctx)
    rn, rmatch, rocc = oracle.search_by_projection(fr.kx, fr.ky, fr.oct, desc, fr.min_x, fr.min_y, fr.inv_w, fr.inv_h, sf, mp["in_view"],
                                                   mp["level"], mp["view_cos"], mp["px"], mp["py"], mp["mp_desc"], mp["has_obs"],
                                                   mp["occupied"], th, 0.8)
    n = len(kps)
    pre = np.where(mp["occupied"], np.arange(n) + 50000, -1).astype("i4")    # features already holding a map point
    qid = (np.arange(len(mp["px"])) * 7 + 3).astype("i4")
    with DeviceFrame(fr, kps["angle"], ctx=ctx) as h:
        for ids in (None, qid):
            h.map_points = pre
            a, b = _sbp_both(m, fr, h, sf, mp, th, ids)
            assert _same(a, b) and b[0] == rn and (b[1] == rmatch).all() and (b[2] == rocc).all() and rn > 300
            new = b[1] >= 0
            want = pre.copy()
            want[new] = b[1][new] if ids is None else ids[b[1][new]]
            assert (h.map_points == want).all()


# ---------------------------------------------------------------------------------------------------------------- 4. frame to frame
@pytest.mark.parametrize("check_ori", [True, False])
def test_handle_search_by_projection_frame(ctx, oracle, check_ori):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    img = synth.frame(2)
    k1, d1 = ex(img)
    hl = DeviceFrame.from_extract(ex, 0, ctx=ctx)                   # the last frame, from its extract
    k2, d2 = ex(np.roll(img, (3, -5), axis=(0, 1)))
    cur = FrameGridView(k2["x"], k2["y"], k2["octave"], d2)
    hc = DeviceFrame.from_extract(ex, 0, ctx=ctx)
    sf = ex.GetScaleFactors()
    rng = np.random.default_rng(4)
    n_last = len(k1)
    last_ids = np.where(rng.random(n_last) < 0.85, rng.permutation(n_last) + 100, -1).astype("i4")
    u = (k1["x"] - 5 + rng.normal(0, 1.0, n_last)).astype("f4"); v = (k1["y"] + 3 + rng.normal(0, 1.0, n_last)).astype("f4")
    valid = (last_ids >= 0) & (u >= 0) & (u <= 752) & (v >= 0) & (v <= 480)
    has_obs = rng.random(n_last) < 0.9
    occupied = np.zeros(len(k2), bool)
    hl.map_points = last_ids
    m = ORBmatcher(0.9, check_ori, ctx=ctx)
    for th in (7.0, 15.0, 40.0):
        ref = m.SearchByProjectionFrame(cur, k2["angle"], sf, valid, u, v, k1["octave"], k1["angle"], d1, has_obs, occupied, th)
        rn, rmatch, rocc = oracle.search_by_projection_frame(cur.kx, cur.ky, cur.oct, d2, k2["angle"], cur.min_x, cur.min_y, cur.inv_w,
                                                             cur.inv_h, sf, valid, u, v, k1["octave"], k1["angle"], d1, has_obs, occupied,
                                                             th, check_ori)
        assert ref[0] == rn and (ref[1] == rmatch).all() and (ref[2] == rocc).all() and rn > 200
        hc.map_points = None
        got = m.SearchByProjectionFrameHandle(hc, hl, sf, valid, u, v, d1, has_obs, occupied, th)
        assert _same(ref, got)
        assert (hc.map_points == np.where(got[1] >= 0, last_ids[np.maximum(got[1], 0)], -1)).all()
        # the relocalisation form: last side as arrays, ids = query_mp_id or the query index
        for qid in (None, last_ids):
            hc.map_points = None
            got = m.SearchByProjectionFrameHandle(hc, None, sf, valid, u, v, d1, has_obs, occupied, th, last_octave=k1["octave"],
                                                  last_angle=k1["angle"], query_mp_id=qid)
            assert _same(ref, got)
            src = np.arange(n_last) if qid is None else qid
            assert (hc.map_points == np.where(got[1] >= 0, src[np.maximum(got[1], 0)], -1)).all()
    hl.close(); hc.close()


# ---------------------------------------------------------------------------------------------------------------- 5. pose
def _pose_frame(seed, n_corr=400, n_free=150):
    """One frame: n_corr features with a map point, n_free without, interleaved; a few wrong matches."""
    g = synth.local_ba_graph(n_free=3, n_fixed=0, n_points=n_corr, seed=seed, max_obs=3)
    rng = np.random.default_rng(seed)
    sel = np.flatnonzero(g["edge_pose"] == 0)
    xyz = g["gt_points"][g["edge_point"][sel]].astype(np.float32).astype(np.float64)
    obs = g["obs"][sel].astype("f4")
    obs[::13] += rng.normal(0, 30, obs[::13].shape).astype("f4")
    k = len(sel)
    n = k + n_free
    has = np.zeros(n, bool); has[rng.choice(n, k, replace=False)] = True
    kx = rng.uniform(0, 752, n).astype("f4"); ky = rng.uniform(0, 480, n).astype("f4")
    kx[has] = obs[:, 0]; ky[has] = obs[:, 1]
    octv = rng.integers(0, 8, n).astype("i4")
    ids = np.full(n, -1, "i4"); ids[has] = rng.permutation(k)       # map-point table order differs from feature order
    table = np.zeros((k, 3)); table[ids[has]] = xyz
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return FrameGridView(kx, ky, octv, desc), ids, table, g["poses"][0], g["intr"][0]


def test_handle_pose_optimize(ctx, oracle):
    is2 = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx).GetInverseScaleSigmaSquares()
    fr, ids, table, pose, intr = _pose_frame(3)
    has = ids >= 0
    pts = table[ids[has]]; obs = np.stack([fr.kx[has], fr.ky[has]], 1).astype("f8"); info = is2[fr.oct[has]].astype("f8")
    rp, ro, rn = Optimizer.PoseOptimizationClient(pose[None], intr[None], np.array([0, has.sum()], "i4"), pts, obs, info, ctx=ctx)
    with DeviceFrame(fr, None, ctx=ctx) as h:
        h.map_points = ids
        p7, outl, ni = Optimizer.PoseOptimizationFrame(h, pose, intr, table, is2)
        assert (p7 == rp[0]).all() and ni == rn[0] and (outl[has] == ro).all() and (outl[~has] == 0).all()
        op, oo, on = oracle.pose_optimize(pose, intr, pts, obs, info)
        assert pose_delta(p7[None], op[None]).max() <= 1e-5 and (outl[has] == oo).all() and ni == on
        assert has.sum() > 300 and outl.sum() >= has.sum() // 13 - 2
        # fewer than 3 correspondences: 0, pose untouched
        two = np.full(h.n, -1, "i4"); two[np.flatnonzero(has)[:2]] = ids[has][:2]
        h.map_points = two
        p7, outl, ni = Optimizer.PoseOptimizationFrame(h, pose, intr, table, is2)
        assert ni == 0 and (p7 == pose).all() and (outl == 0).all()
        # an id outside the table
        bad = ids.copy(); bad[np.flatnonzero(has)[5]] = len(table)
        h.map_points = bad
        with pytest.raises(_lib.CcmError) as e:
            Optimizer.PoseOptimizationFrame(h, pose, intr, table, is2)
        assert e.value.code == E_ARG


@pytest.mark.parametrize("N", C_.FRAME_SIZES)
def test_handle_pose_optimize_at_the_compaction_edges(ctx, N):
    """k_frame_pose_gather is one workgroup of 1024 threads with a ballot per wave and a running base per 1024-block: frames of N
    features at and across 1024, with every feature set, only the last plus two, wave 0 of each block empty, every second 64-group
    empty and exactly 3 set.  Pose, per-feature flags and inlier count equal the array call on the gathered problem bit for bit."""
    is2 = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx).GetInverseScaleSigmaSquares()
    desc = np.random.default_rng(N).integers(0, 256, (N, 32), dtype=np.uint8)
    for pattern in C_.FRAME_PATTERNS:
        fc = C_.frame_case(N, pattern)
        has = fc["mask"]
        pts, obs, info = C_.gathered(fc, is2)
        rp, ro, rn = Optimizer.PoseOptimizationClient(fc["pose"][None], fc["intr"][None], np.array([0, has.sum()], "i4"), pts, obs, info, ctx=ctx)
        with DeviceFrame(FrameGridView(fc["kx"], fc["ky"], fc["oct"], desc, *C_.FRAME_BOUNDS), None, ctx=ctx) as h:
            h.map_points = fc["ids"]
            p7, outl, ni = Optimizer.PoseOptimizationFrame(h, fc["pose"], fc["intr"], fc["table"], is2)
        assert (p7 == rp[0]).all() and ni == rn[0] and (outl[has] == ro).all() and (outl[~has] == 0).all(), (N, pattern)
        assert ni >= 3 and (p7 != fc["pose"]).any() and (has.sum() < 100 or ro.sum() >= has.sum() // 7 - 8), (N, pattern)


# ---------------------------------------------------------------------------------------------------------------- 6. chain
def _chain(ctx, handles, views, angles, sf, is2, world, shift):
    """TrackWithMotionModel then TrackLocalMap for frames 1..3 of `handles`, each step on handles and on host buffers; returns every
    intermediate result of the handle path after asserting it equals the host path."""
    mp_xyz, mp_desc, mp_xy, mp_oct = world
    m = ORBmatcher(0.9, True, ctx=ctx)
    ml = ORBmatcher(0.8, ctx=ctx)
    intr = np.array([458.0, 457.0, 367.0, 248.0])
    n0 = len(views[0].kx)
    ids_prev = np.arange(n0, dtype="i4")                            # frame 0 created the map
    handles[0].map_points = ids_prev
    out = []
    for k in (1, 2, 3):
        cur, last, cv, lv = handles[k], handles[k - 1], views[k], views[k - 1]
        n = len(cv.kx)
        # TrackWithMotionModel: SearchByProjection(Current, Last, 7)
        valid = ids_prev >= 0
        safe = np.maximum(ids_prev, 0)
        u = (lv.kx + shift[1]).astype("f4"); v = (lv.ky + shift[0]).astype("f4")
        valid &= (u >= 0) & (u < 752) & (v >= 0) & (v < 480)
        md = mp_desc[safe]; ho = np.ones(len(u), bool); occ = np.zeros(n, bool)
        cur.map_points = None
        ref = m.SearchByProjectionFrame(cv, angles[k], sf, valid, u, v, lv.oct, angles[k - 1], md, ho, occ, 7.0)
        got = m.SearchByProjectionFrameHandle(cur, last, sf, valid, u, v, md, ho, occ, 7.0)
        assert _same(ref, got) and got[0] > 100
        ids = np.where(got[1] >= 0, ids_prev[np.maximum(got[1], 0)], -1).astype("i4")
        assert (cur.map_points == ids).all()
        # PoseOptimizationClient
        pose = np.array([0, 0, 0, 1, 0, 0, 0], "f8")
        has = ids >= 0
        args = (np.array([0, has.sum()], "i4"), mp_xyz[ids[has]], np.stack([cv.kx[has], cv.ky[has]], 1).astype("f8"), is2[cv.oct[has]].astype("f8"))
        rp, ro, rn = Optimizer.PoseOptimizationClient(pose[None], intr[None], *args, ctx=ctx)
        p7, outl, ni = Optimizer.PoseOptimizationFrame(cur, pose, intr, mp_xyz, is2)
        assert (p7 == rp[0]).all() and ni == rn[0] and (outl[has] == ro).all() and (outl[~has] == 0).all()
        # discard outliers
        ids[outl != 0] = -1
        cur.map_points = ids
        # TrackLocalMap: SearchByProjection(Frame, local map points, th = 1), occupied = features with a map point
        nm = len(mp_xyz)
        px = (mp_xy[:, 0] + shift[1] * k).astype("f4"); py = (mp_xy[:, 1] + shift[0] * k).astype("f4")
        in_view = (px >= 0) & (px < 752) & (py >= 0) & (py < 480)
        in_view[np.isin(np.arange(nm), ids)] = False                 # points already matched are not searched again
        vc = np.full(nm, 0.999, "f4"); ho = np.ones(nm, bool)
        occ = ids >= 0
        refl = ml.SearchByProjection(cv, sf, in_view, mp_oct, vc, px, py, mp_desc, ho, occ, 1.0)
        gotl = ml.SearchByProjectionHandle(cur, sf, in_view, mp_oct, vc, px, py, mp_desc, ho, occ, 1.0)
        assert _same(refl, gotl)
        new = gotl[1] >= 0
        ids[new] = gotl[1][new]
        assert (cur.map_points == ids).all()
        has = ids >= 0
        args = (np.array([0, has.sum()], "i4"), mp_xyz[ids[has]], np.stack([cv.kx[has], cv.ky[has]], 1).astype("f8"), is2[cv.oct[has]].astype("f8"))
        rp2, ro2, rn2 = Optimizer.PoseOptimizationClient(p7[None], intr[None], *args, ctx=ctx)
        p72, outl2, ni2 = Optimizer.PoseOptimizationFrame(cur, p7, intr, mp_xyz, is2)
        assert (p72 == rp2[0]).all() and ni2 == rn2[0] and (outl2[has] == ro2).all()
        out.append((got, p7, outl, ni, gotl, p72, outl2, ni2, ids.copy()))
        ids_prev = ids
    return out


def test_motion_model_chain_on_handles(ctx):
    import torch
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    sf, is2 = ex.GetScaleFactors(), ex.GetInverseScaleSigmaSquares()
    base = synth.frame(5)
    shift = (2, -3)                                               # per frame: rows down 2, columns left 3
    imgs = np.stack([np.roll(base, (shift[0] * k, shift[1] * k), axis=(0, 1)) for k in range(4)])
    dev = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    ex.extract_dev(dev.data_ptr(), 752, 480, 752, 752 * 480, 4)
    kps, desc, counts = ex.fetch()
    views, angles, handles = [], [], []
    for k in range(4):
        n = int(counts[k])
        views.append(FrameGridView(kps[k, :n]["x"], kps[k, :n]["y"], kps[k, :n]["octave"], desc[k, :n]))
        angles.append(kps[k, :n]["angle"].copy())
        handles.append(DeviceFrame.from_extract(ex, k, n=n, ctx=ctx))
    # the map: frame 0's features back-projected at random depths (identity pose)
    rng = np.random.default_rng(9)
    v0 = views[0]
    z = rng.uniform(2, 10, len(v0.kx))
    mp_xyz = np.stack([(v0.kx - 367.0) / 458.0 * z, (v0.ky - 248.0) / 457.0 * z, z], 1).astype(np.float32).astype(np.float64)
    world = (mp_xyz, v0.desc.copy(), np.stack([v0.kx, v0.ky], 1), v0.oct.copy())
    first = _chain(ctx, handles, views, angles, sf, is2, world, shift)
    # another extract on the same context: the handles own their data
    flipped = torch.flip(dev, (2,)).contiguous()
    torch.cuda.synchronize()
    ex.extract_dev(flipped.data_ptr(), 752, 480, 752, 752 * 480, 4)
    ex.fetch()
    again = _chain(ctx, handles, views, angles, sf, is2, world, shift)
    for a, b in zip(first, again):
        assert _same(a[0], b[0]) and (a[1] == b[1]).all() and (a[2] == b[2]).all() and a[3] == b[3]
        assert _same(a[4], b[4]) and (a[5] == b[5]).all() and (a[6] == b[6]).all() and a[7] == b[7] and (a[8] == b[8]).all()
    for h in handles:
        h.close()


# ---------------------------------------------------------------------------------------------------------------- 7. misuse
def test_misuse_returns_error_codes(ctx):
    lib = _lib.load()
    ex, kps, desc = _extract(ctx, 3)
    fr = FrameGridView(kps["x"], kps["y"], kps["octave"], desc)
    sf = ex.GetScaleFactors()
    mp = _map_points(fr, desc, 5)
    m = ORBmatcher(0.8, ctx=ctx)
    other = _lib.Context(0)
    try:
        # from_extract before any extract on this context
        h = C.c_void_p()
        assert lib.ccm_frame_from_extract(other.handle, 0, -1, None, None, 0.0, 0.0, 0.1, 0.1, 75, 48, C.byref(h)) == E_STATE
        # a handle of context A with context B
        with DeviceFrame(fr, kps["angle"], ctx=ctx) as fa:
            mb = ORBmatcher(0.8, ctx=other)
            with pytest.raises(_lib.CcmError) as e:
                mb.SearchByProjectionHandle(fa, sf, mp["in_view"], mp["level"], mp["view_cos"], mp["px"], mp["py"], mp["mp_desc"],
                                            mp["has_obs"], mp["occupied"], 1.0)
            assert e.value.code == E_ARG
        # image out of range
        assert lib.ccm_frame_from_extract(ctx.handle, 1, -1, None, None, 0.0, 0.0, 0.1, 0.1, 75, 48, C.byref(h)) == E_ARG
        assert lib.ccm_frame_from_extract(ctx.handle, -1, -1, None, None, 0.0, 0.0, 0.1, 0.1, 75, 48, C.byref(h)) == E_ARG
        # orientation check against a frame without angles
        with DeviceFrame(fr, None, ctx=ctx) as na, DeviceFrame(fr, kps["angle"], ctx=ctx) as wa:
            n = len(kps)
            args = (sf, np.ones(n, bool), fr.kx, fr.ky, desc, np.ones(n, bool), np.zeros(n, bool), 7.0)
            for cur, last in ((na, wa), (wa, na)):
                with pytest.raises(_lib.CcmError) as e:
                    ORBmatcher(0.9, True, ctx=ctx).SearchByProjectionFrameHandle(cur, last, *args)
                assert e.value.code == E_ARG
            ORBmatcher(0.9, False, ctx=ctx).SearchByProjectionFrameHandle(na, na, *args)   # without the check it runs
    finally:
        other.close()


# ---------------------------------------------------------------------------------------------------------------- 8. fallback
def test_handle_host_acceptance_stays_exact():
    """The host acceptance loops through a handle: a child process with CCM_WINDOW_HOST_ACCEPT=1 reruns the handle matcher tests."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CCM_WINDOW_HOST_ACCEPT="1", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
                          "handle_search_by_projection or construction or chain"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-1000:]


# ---------------------------------------------------------------------------------------------------------------- 9. churn
def test_churn_then_still_exact(ctx, oracle):
    rng = np.random.default_rng(21)
    live = []
    for i in range(1000):
        n = int(rng.integers(0, 3001))
        fr = FrameGridView(rng.uniform(-10, 760, n), rng.uniform(-10, 490, n), rng.integers(0, 8, n), rng.integers(0, 256, (n, 32)))
        live.append(DeviceFrame(fr, rng.uniform(0, 360, n) if i % 2 else None, ctx=ctx))
        if len(live) > 3 or rng.random() < 0.5:                   # a few alive at a time, destroyed out of order
            live.pop(int(rng.integers(0, len(live)))).close()
        if i % 250 == 0 and live:
            first, items = live[-1].grid()
            assert first[-1] == len(items) <= live[-1].n
    for h in live:
        h.close()
    test_handle_search_by_projection(ctx, oracle, 3.0)
