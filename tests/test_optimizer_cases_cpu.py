"""The conditions that make the optimiser GPU tests meaningful, checked on the CPU oracle alone: every case of
tests/optimizer_cases.py is stable under a reversed edge order (so a GPU difference is not conditioning) and reaches the branch of
the schedule it is meant for.  A seed that fails here is replaced in optimizer_cases.py; no GPU test filters a case at run time."""
import numpy as np
import pytest

import optimizer_cases as C
from sim3_problems import make_pose_graph


def _run(oracle, c):
    return oracle.pose_optimize(c["pose"], c["intr"], c["pts"], c["obs"], c["info"])


def _order_stable(oracle, c, tol=C.ORDER_TOL):
    p, o, n = _run(oracle, c)
    p2, o2, n2 = _run(oracle, C.reversed_case(c))
    d = float(np.abs(p - p2).max())
    print("n = %d: %d inliers, pose moves %.3g under a reversed edge order" % (c["n"], n, d))
    assert (o == o2[::-1]).all() and n == n2 and d <= tol, d
    assert np.isfinite(p).all() and n == c["n"] - int(o.sum())
    return p, o, n


@pytest.mark.parametrize("n", C.SIZES_A)
def test_case_a(oracle, n):
    c = C.case_a(n)
    assert len(c["info"]) == n and c["pts"].shape == (n, 3) and c["obs"].shape == (n, 2)
    assert (c["pts"] == C.f32(c["pts"])).all() and (c["obs"] == C.f32(c["obs"])).all() and (c["info"] == C.f32(c["info"])).all()
    p, o, ni = _order_stable(oracle, c)
    assert ni == C.INLIERS_A[n] and (p != c["pose"]).any()
    if n >= 10:
        # case G holds on the oracle: the minimiser is no worse than gt on its own inlier set, and better than the start
        m = o == 0
        at = lambda pose: C.chi2(pose, c["pts"], c["obs"], c["info"], m)
        assert at(p) <= at(c["gt"]) and at(p) < at(c["pose"]), (at(p), at(c["gt"]), at(c["pose"]))


def test_case_a_brackets_the_schedule():
    """The sizes sit on both sides of n < 3, n < 10 (a single round, src/Optimizer.cpp:340-341), the 64-lane wave and the
    256-thread stride, and every frame that has a wrong match loses some edges to it."""
    assert min(C.SIZES_A) == 3 and {9, 10, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025} <= set(C.SIZES_A)
    for n in C.SIZES_A:
        assert 0 < C.INLIERS_A[n] <= n and (n < 7 or C.INLIERS_A[n] < n)        # the wrong matches are found


def test_degenerate_frames(oracle):
    c = C.case_two()
    p, o, n = _run(oracle, c)
    assert n == 0 and (p == c["pose"]).all() and o.sum() == 0
    c = C.empty_case(1)
    p, o, n = _run(oracle, c)
    assert n == 0 and (p == c["pose"]).all() and len(o) == 0


def test_case_c_every_edge_an_outlier(oracle):
    c = C.case_c()
    p, o, n = _order_stable(oracle, c)
    assert n == 0 and o.sum() == 200 and (p == c["pose"]).all()                   # round 1 restarts from the input and finds nothing active


def test_case_d_points_behind_the_camera(oracle):
    c = C.case_d()
    _, z = C.project(c["gt"], c["pts"])
    behind = np.zeros(100, bool); behind[list(C.BEHIND_D)] = True
    assert (z[behind] < -2.5).all() and (z[behind] > -3.5).all() and (z[~behind] > 2).all()
    p, o, n = _order_stable(oracle, c)
    assert n == 95 and (o.astype(bool) == behind).all()


def test_case_e_rank_deficient_and_far_start(oracle):
    c = C.case_e_rank()
    assert (c["pts"] == c["pts"][0]).all() and (c["obs"] == c["obs"][0]).all()
    p, o, n = _order_stable(oracle, c)
    assert n == 50 and o.sum() == 0
    c = C.case_e_far()
    p, o, n = _order_stable(oracle, c, C.ORDER_TOL_FAR)
    assert n == 300 and o.sum() == 0
    assert np.abs(p - c["gt"]).max() <= 2.2e-3 and np.abs(c["pose"] - c["gt"]).max() > 0.1


@pytest.mark.parametrize("N", C.FRAME_SIZES)
def test_frame_cases(oracle, N):
    """The mp_id patterns of the handle-form tests: what each leaves empty, and that the gathered problem is a real optimisation."""
    is2 = oracle.orb_tables(oracle.default_params())["inv_sigma2"]
    want = dict(all=N, last=3, lanes0=N - sum(min(64, N - b) for b in range(0, N, 1024)), alternate=sum(min(64, N - b) for b in range(64, N, 128)), three=3)
    for pattern in C.FRAME_PATTERNS:
        fc = C.frame_case(N, pattern)
        m, ids = fc["mask"], fc["ids"]
        assert m.sum() == want[pattern] and ((ids >= 0) == m).all() and len(set(ids[m])) == m.sum() and ids.max() < N
        groups = np.add.reduceat(m.astype(int), np.arange(0, N, 64))
        if pattern == "last":
            assert m[N - 1] and (groups == 0).sum() >= len(groups) - 3
        if pattern == "lanes0":
            assert (groups[::16] == 0).all() and (np.delete(groups, np.arange(0, len(groups), 16)) > 0).all()
        if pattern == "alternate":
            assert (groups[::2] == 0).all() and (groups[1::2] > 0).all()
        if pattern == "three":
            assert not m[0] and not m[N - 1]
        x0, x1, y0, y1 = C.FRAME_BOUNDS
        assert (fc["kx"] > x0).all() and (fc["kx"] < x1).all() and (fc["ky"] > y0).all() and (fc["ky"] < y1).all()
        pts, obs, info = C.gathered(fc, is2)
        assert (pts == C.f32(pts)).all()
        p, o, n = oracle.pose_optimize(fc["pose"], fc["intr"], pts, obs, info)
        assert n >= 3 and (p != fc["pose"]).any() and (m.sum() < 100 or o.sum() >= m.sum() // 7 - 8), (pattern, n)


def test_sim3_survivor_rule(oracle):
    """12 - nb pairs survive round 0: 10 are optimised, 9 return 0 with the estimate untouched (src/Optimizer.cpp:1022-1023)."""
    for nb, th2, want in zip(C.SIM3_SURVIVOR_NB, C.SIM3_SURVIVOR_TH2, C.SIM3_SURVIVOR_INLIERS):
        p = C.sim3_survivor_problem(nb)
        S, inl, n = oracle.optimize_sim3(p["S0"], 0, p["K1"], p["K2"], p["P1"], p["P2"], p["obs1"], p["obs2"], p["info1"], p["info2"], th2)
        assert n == want and (inl == (np.arange(12) >= nb)).all(), (nb, n, inl)
        assert (S == p["S0"]).all() == (want == 0)


@pytest.fixture(scope="module")
def graph40(oracle):
    sim3, fixed, ei, ej, meas, truth = make_pose_graph(oracle, np.random.default_rng(C.ESS_SEED), n=40)
    return sim3, fixed, ei, ej, meas, truth


def _ess_conditioned(oracle, name, sim3, fixed, ei, ej, meas):
    """The oracle's dense against its block-sparse solver, and against a one-ulp change of one translation: both within C.ESS_COND."""
    try:
        oracle.ess_set_solver(1); ref, info = oracle.essential_graph(sim3, fixed, ei, ej, meas, False, 20)
        oracle.ess_set_solver(2); alt, ainfo = oracle.essential_graph(sim3, fixed, ei, ej, meas, False, 20)
    finally:
        oracle.ess_set_solver(0)
    v = int(np.flatnonzero(fixed == 0)[3])
    moved = sim3.copy(); moved[v, 4] = np.nextafter(moved[v, 4], 10.0)
    ulp, uinfo = oracle.essential_graph(moved, fixed, ei, ej, meas, False, 20)
    d = max(float(np.abs(alt - ref).max()), float(np.abs(ulp - ref).max()))
    print("%s: %d iterations, chi2 %.6g -> %.6g, the oracle moves %.3g" % (name, info["iterations_done"], info["chi2_initial"], info["chi2_final"], d))
    assert info["iterations_done"] == ainfo["iterations_done"] == uinfo["iterations_done"] and d <= C.ESS_COND, (name, d)
    assert (ref[fixed != 0] == sim3[fixed != 0]).all()
    return ref, info


def test_essential_graph_relabelling_and_duplicates(oracle, graph40):
    sim3, fixed, ei, ej, meas, _ = graph40
    ref, rinfo = _ess_conditioned(oracle, "original numbering", sim3, fixed, ei, ej, meas)
    perm = np.random.default_rng(7).permutation(40)
    s2, f2, pi, pj = C.relabel_graph(perm, sim3, fixed, ei, ej)
    assert 40 <= (pi < pj).sum() <= len(ei) - 40                                  # both orientations, plenty of each
    r2, i2 = _ess_conditioned(oracle, "relabelled", s2, f2, pi, pj, meas)
    assert np.abs(r2[perm] - ref).max() <= 1e-12 and i2["iterations_done"] == rinfo["iterations_done"]
    r4, i4 = _ess_conditioned(oracle, "duplicate edges", sim3, fixed, np.tile(ei, 2), np.tile(ej, 2), np.tile(meas, (2, 1)))
    assert np.isclose(i4["chi2_initial"], 2 * rinfo["chi2_initial"], rtol=1e-12) and np.abs(r4 - ref).max() <= 1e-12
    si, sj, sm = C.swap_edges(oracle, ei, ej, meas)
    assert (si < sj).all()
    r3, i3 = _ess_conditioned(oracle, "all edges i < j", sim3, fixed, si, sj, sm)
    assert i3["chi2_final"] < 0.05 * i3["chi2_initial"]


def test_essential_graph_fixed_vertices_and_small_graphs(oracle, graph40):
    sim3, fixed, ei, ej, meas, truth = graph40
    fx = fixed.copy(); fx[20] = 1
    r, i = _ess_conditioned(oracle, "vertices 0 and 20 fixed", sim3, fx, ei, ej, meas)
    assert (r[0] == sim3[0]).all() and (r[20] == sim3[20]).all() and i["chi2_final"] < i["chi2_initial"]
    fm, ci, cj, cm = C.two_chain_graph(oracle, sim3, ei, ej, meas, truth, 20)
    assert len(ci) > 60 and not (((ci > 20) & (cj < 20)) | ((cj > 20) & (ci < 20))).any() and fm.sum() == 1
    r, i = _ess_conditioned(oracle, "two chains", sim3, fm, ci, cj, cm)
    assert (r[20] == sim3[20]).all() and 1e-4 < i["chi2_final"] < 0.5 * i["chi2_initial"]    # a real minimum, not a zero residual
    r, i = oracle.essential_graph(sim3, np.ones(40, np.uint8), ei, ej, meas, False, 20)
    assert (r == sim3).all() and i["chi2_final"] == i["chi2_initial"] and i["iterations_done"] == 0
    s, fx2, e2i, e2j, m2 = C.two_vertex_graph()
    r, i = oracle.essential_graph(s, fx2, e2i, e2j, m2, False, 20)
    assert (r == s).all() and i["chi2_initial"] == 0 and i["chi2_final"] == 0


def test_correct_map_points_restatement(oracle):
    """The float64 numpy restatement against the oracle's Sim3 algebra, point by point."""
    rng = np.random.default_rng(3)
    before = np.stack([C.rand_sim3(rng) for _ in range(5)]); after = np.stack([C.rand_sim3(rng) for _ in range(5)])
    pts = rng.normal(0, 3, (20, 3)); refv = rng.integers(-1, 5, 20)
    out = C.correct_map_points_ref(pts, refv, before, after)
    for k in range(20):
        if refv[k] < 0:
            assert (out[k] == pts[k]).all()
            continue
        comp = oracle.sim3_mul(oracle.sim3_inverse(after[refv[k]]), before[refv[k]])
        exp = comp[7] * (C.quat_R(comp[:4]) @ pts[k]) + comp[4:7]
        assert np.abs(out[k] - exp).max() < 1e-13
