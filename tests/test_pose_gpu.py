"""Batched Optimizer::PoseOptimizationClient on the GPU vs the CPU oracle."""
import numpy as np
import pytest

import optimizer_cases as C
from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.optimizer import Optimizer, pose_delta

pytestmark = pytest.mark.gpu


def _frames(seed, n_frames=12, n_points=1500, outlier_every=13):
    g = synth.local_ba_graph(n_free=n_frames, n_fixed=0, n_points=n_points, seed=seed, max_obs=n_frames)
    poses, intr, first, pts, obs, info = [], [], [0], [], [], []
    rng = np.random.default_rng(seed)
    for p in range(n_frames):
        sel = np.flatnonzero(g["edge_pose"] == p)
        pw = g["gt_points"][g["edge_point"][sel]].astype(np.float32).astype(np.float64)   # MapPoint positions are float32
        ob = g["obs"][sel].copy()
        ob[::outlier_every] += rng.normal(0, 30, ob[::outlier_every].shape).astype(np.float32)   # wrong matches
        poses.append(g["poses"][p]); intr.append(g["intr"][p])
        pts.append(pw); obs.append(ob); info.append(g["info"][sel]); first.append(first[-1] + len(sel))
    return (np.asarray(poses), np.asarray(intr), np.asarray(first, "i4"), np.concatenate(pts), np.concatenate(obs),
            np.concatenate(info), g["gt_poses"])


def test_pose_optimization_matches_oracle(ctx, oracle):
    poses, intr, first, pts, obs, info, gt = _frames(3)
    out, outl, ninl = Optimizer.PoseOptimizationClient(poses, intr, first, pts, obs, info, ctx=ctx)
    for f in range(len(poses)):
        a, b = first[f], first[f + 1]
        rp, ro, rn = oracle.pose_optimize(poses[f], intr[f], pts[a:b], obs[a:b], info[a:b])
        assert pose_delta(out[f:f + 1], rp[None]).max() <= 1e-5
        assert (outl[a:b] == ro).all() and ninl[f] == rn
        assert pose_delta(out[f:f + 1], gt[f:f + 1]).max() < pose_delta(poses[f:f + 1], gt[f:f + 1]).max()
        assert ro.sum() >= (b - a) // 13 - 2           # the injected wrong matches are found


def test_pose_optimization_edge_cases(ctx, oracle):
    poses, intr, first, pts, obs, info, _ = _frames(5, n_frames=4, n_points=200)
    # frame 0: fewer than 3 correspondences -> untouched, returns 0; frame 1: fewer than 10 -> a single round
    cut = [2, 8, first[3] - first[2], first[4] - first[3]]
    sel = np.concatenate([np.arange(first[f], first[f] + cut[f]) for f in range(4)])
    f2 = np.concatenate([[0], np.cumsum(cut)]).astype("i4")
    out, outl, ninl = Optimizer.PoseOptimizationClient(poses, intr, f2, pts[sel], obs[sel], info[sel], ctx=ctx)
    assert ninl[0] == 0 and (out[0] == poses[0]).all()
    for f in range(1, 4):
        a, b = f2[f], f2[f + 1]
        rp, ro, rn = oracle.pose_optimize(poses[f], intr[f], pts[sel][a:b], obs[sel][a:b], info[sel][a:b])
        assert pose_delta(out[f:f + 1], rp[None]).max() <= 1e-5 and (outl[a:b] == ro).all() and ninl[f] == rn
    # a batch of 256 frames: every frame equals its single-frame result
    poses, intr, first, pts, obs, info, _ = _frames(7, n_frames=16, n_points=1200)
    reps = 16
    P = np.tile(poses, (reps, 1)); K = np.tile(intr, (reps, 1))
    F = np.concatenate([[0], np.cumsum(np.tile(np.diff(first), reps))]).astype("i4")
    out, outl, ninl = Optimizer.PoseOptimizationClient(P, K, F, np.tile(pts, (reps, 1)), np.tile(obs, (reps, 1)), np.tile(info, reps), ctx=ctx)
    one, outl1, ninl1 = Optimizer.PoseOptimizationClient(poses, intr, first, pts, obs, info, ctx=ctx)
    assert (out == np.tile(one, (reps, 1))).all() and (ninl == np.tile(ninl1, reps)).all() and (outl == np.tile(outl1, reps)).all()


# ---------------------------------------------------------------------------------------------------------------- schedule edges
# One-frame problems of a chosen size (tests/optimizer_cases.py; tests/test_optimizer_cases_cpu.py holds the oracle alone to the
# conditions that make them meaningful).  Flags and inlier counts must be equal, max |pose7 - oracle pose7| <= C.POSE_TOL = 1e-8:
# three orders above what a reversed edge order does to the oracle (<= 1e-10), left for the device's sqrt / pow / sin / cos.
# Measured on an MI355X: at most 8.0e-10 (A, n = 4); every other case of A to E stays below 1e-11.


def _gpu(ctx, cases):
    out, outl, ninl = Optimizer.PoseOptimizationClient(*C.batch(cases), ctx=ctx)
    first = np.concatenate([[0], np.cumsum([len(c["info"]) for c in cases])])
    return [(out[f], outl[first[f]:first[f + 1]], int(ninl[f])) for f in range(len(cases))]


def _same(a, b):
    return (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]


@pytest.fixture(scope="module")
def case_a(ctx, oracle):
    """n -> (case, oracle result, single-frame GPU result), computed once and left unchanged."""
    res = {}
    for n in C.SIZES_A:
        c = C.case_a(n)
        res[n] = (c, oracle.pose_optimize(c["pose"], c["intr"], c["pts"], c["obs"], c["info"]), _gpu(ctx, [c])[0])
    return res


def _against_oracle(name, c, ref, got, tol=C.POSE_TOL):
    d = float(np.abs(got[0] - ref[0]).max())
    print("%s: %d inliers of %d, max |pose7 - oracle| = %.3g" % (name, got[2], len(c["info"]), d))
    assert (got[1] == ref[1]).all() and got[2] == ref[2], name
    assert d <= tol, (name, d)


@pytest.mark.parametrize("n", C.SIZES_A)
def test_pose_stride_and_schedule_boundaries(case_a, n):
    """A. n = 3 is the smallest optimised frame, 9 / 10 the single-round rule, the rest sit on either side of the wave and the stride."""
    c, ref, got = case_a[n]
    _against_oracle("A n=%d" % n, c, ref, got)
    assert got[2] == C.INLIERS_A[n]


def test_pose_batch_with_empty_frames_equals_single_frames(ctx, case_a):
    """B. the 15 frames of A in one launch, an empty frame first and last and a 2-correspondence frame in the middle."""
    cases = [case_a[n][0] for n in C.SIZES_A]
    cases = [C.empty_case(1)] + cases[:7] + [C.case_two()] + cases[7:] + [C.empty_case(2)]
    first = C.batch(cases)[2]
    assert first[0] == first[1] and first[-1] == first[-2] and first[9] - first[8] == 2
    got = _gpu(ctx, cases)
    for c, g in zip(cases, got):
        if len(c["info"]) < 3:
            assert g[2] == 0 and (g[0] == c["pose"]).all() and (g[1] == 0).all()
        else:
            assert _same(g, case_a[len(c["info"])][2]), len(c["info"])


def test_pose_every_edge_an_outlier_after_round_0(ctx, oracle):
    """C. round 1 restarts from the input pose and finds nothing active: the any_active == 0 exit."""
    c = C.case_c()
    ref = oracle.pose_optimize(c["pose"], c["intr"], c["pts"], c["obs"], c["info"])
    got = _gpu(ctx, [c])[0]
    _against_oracle("C", c, ref, got)
    assert got[2] == 0 and got[1].sum() == 200 and (got[0] == c["pose"]).all()


def test_pose_points_behind_the_camera(ctx, oracle):
    """D. five map points with a negative camera-frame depth: flagged, the other 95 kept."""
    c = C.case_d()
    ref = oracle.pose_optimize(c["pose"], c["intr"], c["pts"], c["obs"], c["info"])
    got = _gpu(ctx, [c])[0]
    _against_oracle("D", c, ref, got)
    assert got[2] == 95 and list(np.flatnonzero(got[1])) == list(C.BEHIND_D)


def test_pose_rank_deficient_and_far_start(ctx, oracle):
    """E. 50 copies of one correspondence (only lambda makes H positive definite), and a clean frame started far from gt."""
    c = C.case_e_rank()
    ref = oracle.pose_optimize(c["pose"], c["intr"], c["pts"], c["obs"], c["info"])
    got = _gpu(ctx, [c])[0]
    _against_oracle("E rank", c, ref, got)
    assert got[2] == 50 and got[1].sum() == 0
    c = C.case_e_far()
    ref = oracle.pose_optimize(c["pose"], c["intr"], c["pts"], c["obs"], c["info"])
    got = _gpu(ctx, [c])[0]
    _against_oracle("E far", c, ref, got)
    assert got[2] == 300 and np.abs(got[0] - c["gt"]).max() <= 2.2e-3


def test_pose_history_independence(case_a):
    """F. the per-edge error and flag buffers of a context are reused and never cleared: a small frame after a large one and after
    a frame that left every flag set must equal the same frame on a fresh context, bit for bit."""
    c11, big, allout = case_a[11][0], case_a[1025][0], C.case_c()
    fresh = _lib.Context(0)
    try:
        want = _gpu(fresh, [c11])[0]
    finally:
        fresh.close()
    used = _lib.Context(0)
    try:
        _gpu(used, [big])
        first = _gpu(used, [c11])[0]
        assert _gpu(used, [allout])[0][2] == 0
        second = _gpu(used, [c11])[0]
    finally:
        used.close()
    assert _same(first, want) and _same(second, want)
    assert _same(want, case_a[11][2])


@pytest.mark.parametrize("n", [n for n in C.SIZES_A if n >= 10])
def test_pose_is_a_minimiser_independent_of_the_oracle(case_a, n):
    """G. float64 numpy chi2 over the final inlier set: a minimiser is no worse than any other pose, gt and the start included."""
    c, _, got = case_a[n]
    m = got[1] == 0
    at = lambda pose: C.chi2(pose, c["pts"], c["obs"], c["info"], m)
    print("G n=%d: chi2 / chi2(gt) = %.4f, chi2 / chi2(start) = %.4g" % (n, at(got[0]) / at(c["gt"]), at(got[0]) / at(c["pose"])))
    assert at(got[0]) <= at(c["gt"]) and at(got[0]) < at(c["pose"])
