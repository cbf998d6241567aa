"""The conditions that make the BA case tests meaningful, checked on the CPU oracle and in numpy alone: every case of
tests/ba_cases.py reaches the size rule it is meant for, the oracle's result on it does not depend on the edge order or on which of
its two solvers runs (so a GPU difference is not conditioning), the oracle's first iteration is the numpy definition `one_step`, and
`one_step` agrees with central differences of its own residual.  A seed that fails here is replaced in ba_cases.py (RESEEDED); no
GPU test filters a case at run time.  Run with -s for the table of rules reached and sensitivities measured."""
from collections import Counter

import numpy as np
import pytest

import ba_cases as B

# name -> nfree, n = 6 nfree, n <= 138 (k_dense_small_solve), pitch (n rounded up to 48), nc = 7 ceil(nfree / 16), landmarks, edges.
# Written out by hand, not through ba_cases.rules: these are the targets.
EXPECT = {
    "D1": (1, 6, True, 48, 7, 120, 360), "D2": (2, 12, True, 48, 7, 120, 480), "D22": (22, 132, True, 144, 14, 144, 864),
    "D23-full": (23, 138, True, 144, 14, 196, 1176), "D23-band": (23, 138, True, 144, 14, 150, 900),
    "D23-isolated": (23, 138, True, 144, 14, 150, 900),
    "D24-full": (24, 144, False, 144, 14, 206, 1236), "D24-band": (24, 144, False, 144, 14, 156, 936),
    "D24-isolated": (24, 144, False, 144, 14, 156, 936), "D25": (25, 150, False, 192, 14, 162, 972),
    "D255": (255, 1530, False, 1536, 112, 1542, 9252), "D256": (256, 1536, False, 1536, 112, 1548, 9288),
    "D257": (257, 1542, False, 1584, 119, 1554, 9324),
    "D23-one-fixed": (23, 138, True, 144, 14, 144, 864), "D257-one-fixed": (257, 1542, False, 1584, 119, 1548, 9288),
    "L60": (60, 360, False, 384, 28, 80, 1970),
    "L-31-landmarks": (3, 18, True, 48, 7, 31, 124), "L-32-landmarks": (3, 18, True, 48, 7, 32, 128),
    "L-33-landmarks": (3, 18, True, 48, 7, 33, 132),
    "L-255-edges": (6, 36, True, 48, 7, 51, 255), "L-256-edges": (6, 36, True, 48, 7, 51, 256), "L-257-edges": (6, 36, True, 48, 7, 51, 257),
    "S10": (10, 60, True, 96, 7, 120, 600), "S30": (30, 180, False, 192, 14, 192, 960),
    "P1": (1, 6, True, 48, 7, 120, 360), "P7": (7, 42, True, 48, 7, 120, 720), "P8": (8, 48, True, 48, 7, 120, 720),
    "P9": (9, 54, True, 96, 7, 120, 720), "P17": (17, 102, True, 144, 14, 120, 720), "P31": (31, 186, False, 192, 14, 198, 1188),
    "P32": (32, 192, False, 192, 14, 204, 1224), "P33": (33, 198, False, 240, 21, 210, 1260),
    "P144": (144, 864, False, 864, 63, 876, 5256), "P145": (145, 870, False, 912, 70, 882, 5292),
    "P161": (161, 966, False, 1008, 77, 978, 5868),
}

_RUNS = {}


def _runs(oracle, name):
    """The oracle on a case, per schedule: with the dense solver (what it picks by itself below 400 free keyframes), with the
    block-sparse solver, and with the block-sparse solver on the reversed edge list."""
    if name not in _RUNS:
        g = B.case(name)
        out = {}
        for label, its, huber, its2 in B.SCHEDULES:
            try:
                oracle.ba_set_solver(1); dense = oracle.ba_solve(g, its, huber, its2)
                oracle.ba_set_solver(2); sparse = oracle.ba_solve(g, its, huber, its2)
                rev = oracle.ba_solve(B.reversed_edges(g), its, huber, its2)
            finally:
                oracle.ba_set_solver(0)
            out[label] = (sparse, rev, dense)
        _RUNS[name] = out
    return _RUNS[name]


def _moved(a, b):
    return max(float(np.abs(a["poses"] - b["poses"]).max()), float(np.abs(a["points"] - b["points"]).max()))


def test_the_case_list_is_the_one_asked_for():
    sizes = lambda table: sorted(v[0] for v in table.values())
    assert sizes(B.D_SMALL) == [1, 2, 22, 23, 23, 23, 24, 24, 24, 25] and sizes(B.D_LARGE) == [255, 256, 257]
    assert sorted((v[0], v[2]) for v in B.D_ONE_FIXED.values()) == [(23, 1), (257, 1)]
    for n in (23, 24):
        assert {v[1] for v in B.D_SMALL.values() if v[0] == n} == {"full", "band", "isolated"}
    assert sorted(B.L_ROWS) == sorted([(0, 2), (0, 4), (1, 1)] + [(k, 0) for k in (2, 7, 8, 9, 15, 16, 17, 47, 48, 49, 56, 60)] + [(48, 4)])
    assert B.P_SIZES == (1, 7, 8, 9, 17, 31, 32, 33, 144, 145, 161) and set(B.S_CASES) == {"S10", "S30"}
    assert set(EXPECT) == set(B.ALL_CASES)


@pytest.mark.parametrize("name", B.ALL_CASES)
def test_case_reaches_its_rule(name):
    g = B.case(name)
    nfree, n, small, pitch, nc, L, E = EXPECT[name]
    ru = B.rules(g)
    got = (ru["nfree"], ru["n"], ru["small"], ru["pitch"], ru["nc"], len(g["points"]), len(g["edge_pose"]))
    print("%-15s nfree %3d  n %4d  %s  pitch %4d  nc %3d (coarse %s)  %4d landmarks  %4d edges" %
          (name, nfree, n, "small " if small else ("PCG   " if ru["pcg"] else "dense "), pitch, nc, "on" if ru["coarse"] else "off", L, E))
    assert got == (nfree, n, small, pitch, nc, L, E), got
    n_fixed = int((g["fixed"] != 0).sum())
    assert n_fixed == (1 if name in B.D_ONE_FIXED else 4 if name == "L60" else 2)
    assert ru["pcg"] == (nfree >= 257) and ru["coarse"] == (nfree >= 145)
    free, total = B.edge_counts(g)
    lists = Counter(zip(free.tolist(), (total - free).tolist()))
    P = len(g["poses"])
    if name == "L60":
        assert lists == Counter({row: B.L_REPEAT for row in B.L_ROWS})              # exactly k free + f fixed edges, 5 landmarks each
        assert {int(np.ceil(t / B.LM_LANES)) for t in total} == {1, 2, 3, 6, 7, 8}   # trips of the 8-lane landmark kernels
        # every landmark of the row form has a neighbour in its workgroup that enumerates from LDS
        from_lds = lambda q, p: 0 <= p < L and 0 < free[p] <= B.SP_PF_CAP and q // B.LM_PER_WG == p // B.LM_PER_WG
        for q in np.flatnonzero(free > B.SP_PF_CAP):
            assert from_lds(q, q + 1) or from_lds(q, q - 1), q
    elif name.endswith("-landmarks"):
        assert (total == 4).all() and L in (B.LM_PER_WG - 1, B.LM_PER_WG, B.LM_PER_WG + 1)
    elif name.endswith("-edges"):
        assert sorted(Counter(total.tolist()).items()) == {255: [(5, 51)], 256: [(5, 50), (6, 1)], 257: [(5, 49), (6, 2)]}[E] and E in (255, 256, 257)
    elif name in B.S_CASES:
        assert (total == 5).all() and g["moved"].sum() == 5 + (g["edge_pose"] == B.stranded_keyframe(nfree)).sum() - int(
            ((g["edge_point"] == 0) & (g["edge_pose"] == B.stranded_keyframe(nfree))).sum())
    else:
        assert (total == min(6, P)).all() and L >= max(120, 6 * P)
    per_kf = np.bincount(g["edge_pose"], minlength=P)
    sc = B.structure_counts(g)
    if name.endswith("-isolated"):
        iso = B.isolated_keyframe(nfree)
        assert per_kf[iso] == 0 and g["fixed"][iso] == 0 and (np.delete(per_kf, iso) >= 6).all()
    else:
        assert (per_kf[g["fixed"] == 0] >= 6).all()
    if name.endswith("-full"):
        assert sc["schur_blocks"] == nfree * (nfree + 1) // 2                         # every lower tile of k_dense_small_solve has a block
    if name.endswith("-band"):
        assert sc["schur_blocks"] == sum(min(6, nfree - a) for a in range(nfree))     # bandwidth 5: most tiles have none


@pytest.mark.parametrize("name", B.ALL_CASES)
def test_structure_counts_against_enumeration(name):
    g = B.case(name)
    col = {int(p): i for i, p in enumerate(np.flatnonzero(g["fixed"] == 0))}
    per_lm = {}
    for p, q in zip(g["edge_pose"].tolist(), g["edge_point"].tolist()):
        if p in col:
            per_lm.setdefault(q, []).append(col[p])
    pairs, blocks = 0, {(a, a) for a in range(len(col))}
    for f in per_lm.values():
        for i, a in enumerate(f):
            for b in f[i:]:
                pairs += 1; blocks.add((min(a, b), max(a, b)))
    assert B.structure_counts(g) == dict(schur_pairs=pairs, schur_blocks=len(blocks))


@pytest.mark.parametrize("name", B.ALL_CASES)
def test_oracle_does_not_depend_on_edge_order_or_solver(oracle, name):
    """Admissibility: within ORDER_TOL and with equal trial counts under both changes.  The measured sensitivities are the ones
    ba_cases.SENS records; the GPU bounds are derived from those."""
    g = B.case(name)
    s_lam = 0.0
    for k, (label, *_rest) in enumerate(B.SCHEDULES):
        r, rev, dense = _runs(oracle, name)[label]
        s = max(_moved(r, rev), _moved(dense, r))
        lam = max(abs(x["lambda_final"] / r["lambda_final"] - 1.0) for x in (rev, dense))
        s_lam = max(s_lam, lam)
        print("%-15s %-7s %2d iterations %2d trials, chi2 %.6g -> %.6g, %3d outliers; moves %.2e (order) %.2e (solver), lambda %.2e" %
              (name, label, r["iterations_done"], r["trials"], r["chi2_initial"], r["chi2_final"], int(r["outlier"].sum()),
               _moved(r, rev), _moved(dense, r), lam))
        assert np.isfinite(r["poses"]).all() and np.isfinite(r["points"]).all()
        for x in (rev, dense):
            assert x["trials"] == r["trials"] and x["iterations_done"] == r["iterations_done"]
        assert (rev["outlier"][::-1] == r["outlier"]).all() and (dense["outlier"] == r["outlier"]).all()
        assert s <= B.ORDER_TOL, (label, s)
        assert s <= B.SENS[name][1 + k], (label, s, B.SENS[name])                       # what the GPU bound was derived from
        assert r["chi2_final"] < r["chi2_initial"] and (r["poses"][g["fixed"] != 0] == g["poses"][g["fixed"] != 0]).all()
    assert s_lam <= B.SENS[name][3], (s_lam, B.SENS[name])


@pytest.mark.parametrize("name", tuple(B.S_CASES))
def test_s_cases_strand_a_keyframe_and_a_landmark(oracle, name):
    g = B.case(name)
    r = _runs(oracle, name)["local"][0]
    kf = B.stranded_keyframe(B.rules(g)["nfree"])
    assert r["outlier"][g["moved"]].all() and r["outlier"][g["edge_pose"] == kf].all() and r["outlier"][g["edge_point"] == 0].all()
    assert r["iterations_done"] < 15
    # the second stage leaves their blocks to lambda alone: neither moves after the first stage
    r1 = oracle.ba_solve(g, 5, B.HUBER_LOCAL)
    assert np.abs(r["poses"][kf] - r1["poses"][kf]).max() < 1e-12 and np.abs(r["points"][0] - r1["points"][0]).max() < 1e-12
    assert (r1["poses"][kf] != g["poses"][kf]).any()


# ------------------------------------------------------------------------------------------------------------ one_step
def test_one_step_jacobians_are_the_derivatives_of_its_residual():
    """Central differences of `residuals` under pose <- exp(eps e_i) pose and point <- point + eps e_j, at 1e-6 of the largest entry."""
    g = B.case("L-33-landmarks")
    R, t = B.pose_Rt(g["poses"]); X = g["points"].copy()
    err, Xc = B.residuals(g, R, t, X)
    Jp, Jl = B.jacobians(g, R, Xc)
    eps = 1e-6
    worst = 0.0
    for i in range(6):
        d = np.zeros(6); d[i] = eps
        side = []
        for sgn in (1, -1):
            dR, dt = B.se3_exp(sgn * d)
            side.append(B.residuals(g, np.einsum("ij,pjk->pik", dR, R), t @ dR.T + dt, X)[0])
        worst = max(worst, float(np.abs((side[0] - side[1]) / (2 * eps) - Jp[:, :, i]).max()))
    for j in range(3):
        d = np.zeros(3); d[j] = eps
        num = (B.residuals(g, R, t, X + d)[0] - B.residuals(g, R, t, X - d)[0]) / (2 * eps)
        worst = max(worst, float(np.abs(num - Jl[:, :, j]).max()))
    scale = max(float(np.abs(Jp).max()), float(np.abs(Jl).max()))
    print("one_step Jacobians against central differences: %.2e of the largest entry %.4g" % (worst / scale, scale))
    assert worst <= 1e-6 * scale


@pytest.mark.parametrize("huber", [0.0, B.HUBER_GLOBAL])
def test_one_step_against_a_numerical_gauss_newton_step(huber):
    """The whole step once more from the stacked residual alone: its Jacobian by central differences over every unknown, the Huber
    weights, lambda, one solve.  Agrees with one_step to what the differences allow."""
    g = B.case("L-31-landmarks")
    R, t = B.pose_Rt(g["poses"]); X = g["points"].copy()
    free = np.flatnonzero(g["fixed"] == 0)
    F, L = len(free), len(X)
    n = 6 * F + 3 * L

    def res(x):
        R1, t1 = R.copy(), t.copy()
        for k, p in enumerate(free):
            dR, dt = B.se3_exp(x[6 * k:6 * k + 6])
            R1[p] = dR @ R[p]; t1[p] = dR @ t[p] + dt
        return B.residuals(g, R1, t1, X + x[6 * F:].reshape(L, 3))[0].ravel()
    eps = 1e-6
    J = np.zeros((2 * len(g["obs"]), n))
    for i in range(n):
        d = np.zeros(n); d[i] = eps
        J[:, i] = (res(d) - res(-d)) / (2 * eps)
    e0 = res(np.zeros(n)).reshape(-1, 2)
    c2 = g["info"] * (e0 ** 2).sum(1)
    w = np.where((huber <= 0) | (c2 <= huber * huber), 1.0, huber / np.sqrt(np.maximum(c2, 1e-300))) * g["info"]
    W = np.repeat(w, 2)
    H = J.T @ (W[:, None] * J); b = -J.T @ (W * e0.ravel())
    lam = 1e-5 * np.diag(H).max()
    x = np.linalg.solve(H + lam * np.eye(n), b)
    a = B.one_step(g, huber)
    assert (w < g["info"]).any() == (huber > 0)                                     # the kernel bites on some edge
    assert a["trials"] == 1 and np.isclose(a["lam"], lam, rtol=1e-8)
    assert np.abs(a["points"] - (X + x[6 * F:].reshape(L, 3))).max() <= 1e-6 * np.abs(x).max()
    for k, p in enumerate(free):
        dR, dt = B.se3_exp(x[6 * k:6 * k + 6])
        assert np.abs(a["R"][p] - dR @ R[p]).max() <= 1e-6 * np.abs(x).max() and np.abs(a["t"][p] - (dR @ t[p] + dt)).max() <= 1e-6 * np.abs(x).max()


@pytest.mark.parametrize("name", B.ONE_STEP_CASES)
def test_oracle_first_iteration_is_one_step(oracle, name):
    """The yardstick held to the definition, on lists of 49 and more observations and on a keyframe without edges too; lambda_final
    is lambda / 3 after the accepted step.  s: one_step's own change under a reversed edge list, which must let the case into the GPU
    check (<= ORDER_TOL) and is what ba_cases.SENS records."""
    g = B.case(name)
    fixed = g["fixed"] != 0
    s = 0.0
    for huber in (0.0, B.HUBER_GLOBAL):
        a = B.one_step(g, huber)
        rev = B.one_step(B.reversed_edges(g), huber)
        s = max(s, max(float(np.abs(a[k] - rev[k]).max()) for k in ("R", "t", "points")))
        r = oracle.ba_solve(g, 1, huber)
        R, t = B.pose_Rt(r["poses"])
        d = (float(np.abs(R - a["R"]).max()), float(np.abs(t - a["t"]).max()), float(np.abs(r["points"] - a["points"]).max()))
        print("%-15s huber %.3f: oracle - one_step |dR| %.2e |dt| %.2e |dX| %.2e, lambda %.6g" % ((name, huber) + d + (a["lam"],)))
        assert r["trials"] == a["trials"] and r["iterations_done"] == 1
        assert max(d) <= B.ONE_STEP_ORACLE_TOL, d
        if name in B.S_CASES and huber == 0.0:
            # without a kernel the moved edges make the first trials fail: the definition and the oracle reject the same ones, and the
            # accepted one scales lambda by its own rho
            assert a["trials"] > 1 and np.isclose(r["lambda_final"], a["lam_final"], rtol=1e-9, atol=0)
        else:
            assert a["trials"] == 1 and a["lam_final"] == a["lam"] * (1.0 / 3.0)
            assert np.isclose(r["lambda_final"], a["lam"] / 3.0, rtol=1e-12, atol=0)
        assert (a["R"][fixed] == B.pose_Rt(g["poses"])[0][fixed]).all() and (a["t"][fixed] == g["poses"][fixed, 4:]).all()
    print("%-15s one_step moves %.2e under a reversed edge list" % (name, s))
    assert s <= B.ORDER_TOL and s <= B.SENS[name][0], (s, B.SENS[name])


def test_size_rules_are_the_ones_in_the_sources():
    """ba_cases.py restates the kernels' size rules; a rule that changes in the sources must change there too, or the cases stop
    sitting on it without anybody noticing."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "motioncheck_ccm_slam_amd", "csrc")

    def found(fname, pattern):
        with open(os.path.join(csrc, fname)) as f:
            m = re.search(pattern, f.read())
        assert m, (fname, pattern)
        return int(m.group(1))
    assert found("ba_dense.hip", r"#define DENSE_SMALL_MAX (\d+)") == B.DENSE_SMALL_MAX
    assert found("ba_dense.hip", r"#define DS_TPB (\d+)") == 576                    # two threads per tile: 23 keyframes = 276 tiles
    assert found("ba_dense.hip", r"#define INV_B (\d+)") == B.INV_B
    assert found("ba_host.cpp", r'num\("CCM_BA_DENSE_MAX", (\d+)\)') == B.DENSE_MAX
    assert found("ba_host.cpp", r"env\.want_coarse && nc >= (\d+) &&") == B.COARSE_MIN
    assert found("ba_pcg.h", r"#define PCG_CL (\d+)") * found("ba_pcg.h", r"#define PCG_AGG (\d+)") == B.AGG_KF
    assert found("ba_pcg.h", r"#define PCG_CDOF (\d+)") == B.CDOF
    assert found("ba_pcg.h", r"#define PCG_UPD_TPB (\d+)") == 6 * 32                # the 32-keyframe update block of the P sizes
    assert found("ba_structure.hip", r"#define SP_PF_CAP (\d+)") == B.SP_PF_CAP
    assert found("ba_structure.hip", r"#define SP_PF_LANES (\d+)") == B.LM_LANES
    assert found("ba_kernels.hip", r"#define BA_LM_LANES (\d+)") == B.LM_LANES
