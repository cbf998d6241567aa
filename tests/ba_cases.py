"""Bundle-adjustment graphs that sit on the size rules of the BA kernels, and a definition of one Levenberg iteration that owes
nothing to the oracle.  Unlike synth.local_ba_graph, `graph` gives every landmark exactly the observation list it is asked for, so
the cases can sit on DENSE_SMALL_MAX / INV_B (ba_dense.hip), CCM_BA_DENSE_MAX and the coarse level's nc >= 64 (ba_host.cpp), PCG_CL /
PCG_UPD_KF (ba_pcg.h), SP_PF_CAP / SP_PF_LANES (ba_structure.hip) and BA_LM_LANES (ba_kernels.hip).
tests/test_ba_cases_cpu.py checks on the CPU oracle that every case listed here reaches the rule it is meant for and is stable under
a reversed edge order and a change of the oracle's solver; tests/test_ba_cases_gpu.py runs them on the GPU.
A plain module: no fixtures, nothing that needs a GPU."""
import numpy as np

from motioncheck_ccm_slam_amd import synth

HUBER_GLOBAL = float(np.float32(np.sqrt(5.99)))      # src/Optimizer.cpp:81
HUBER_LOCAL = float(np.float32(np.sqrt(5.991)))      # src/Optimizer.cpp:468

# the rules the cases sit on, as the sources state them
DENSE_SMALL_MAX = 138      # ba_dense.hip: n = 6 nfree <= 138 -> k_dense_small_solve
INV_B = 48                 # ba_dense.hip: the blocked inverse works on a pitch rounded up to 48
DENSE_MAX = 1536           # ba_host.cpp: default CCM_BA_DENSE_MAX, n above it -> PCG
AGG_KF = 16                # ba_pcg.h: PCG_CL 8 keyframes per cluster, PCG_AGG 2 clusters per aggregate
CDOF = 7                   # ba_pcg.h: coarse unknowns per aggregate
COARSE_MIN = 64            # ba_host.cpp: the coarse level is on from nc >= 64
SP_PF_CAP = 48             # ba_structure.hip: more free edges than this -> row form of the pair enumeration
LM_LANES = 8               # ba_kernels.hip (BA_LM_LANES), ba_structure.hip (SP_PF_LANES): lanes that share a landmark
LM_PER_WG = 32             # 256 threads / 8 lanes


def rules(g):
    """Where a graph falls under the size rules above."""
    nfree = int((g["fixed"] == 0).sum())
    n = 6 * nfree
    nc = CDOF * ((nfree + AGG_KF - 1) // AGG_KF)
    return dict(nfree=nfree, n=n, small=n <= DENSE_SMALL_MAX, pitch=(n + INV_B - 1) // INV_B * INV_B, pcg=n > DENSE_MAX,
                nc=nc, nc_pitch=(nc + INV_B - 1) // INV_B * INV_B, coarse=nc >= COARSE_MIN)


# ------------------------------------------------------------------------------------------------------------ graphs
def fixed_mask(n_free, n_fixed):
    """The fixed keyframes spread evenly over the arc (2: the first and the last; 1: the first)."""
    P = n_free + n_fixed
    fixed = np.zeros(P, bool)
    fixed[np.unique(np.linspace(0, P - 1, n_fixed).round().astype(int))] = True
    assert fixed.sum() == n_fixed
    return fixed


def graph(n_free, n_fixed, obs_sets, seed, sigma=(0.01, 0.03, 0.03)):
    """Keyframes on config 4's arc (synth.local_ba_graph); landmark q is observed by exactly the keyframes obs_sets[q].  The
    landmarks lie in a box compact enough to be in every image.  sigma: start error of rotation (rad), translation and points (m)."""
    rng = synth.SplitMix64(seed)
    P = n_free + n_fixed
    ang = np.linspace(-0.6, 0.6, P)
    cams = np.stack([3.0 * np.sin(ang), -3.0 * np.cos(ang), 0.15 * np.sin(3 * ang)], 1)
    Rs, ts = [], []
    for i in range(P):
        R = synth._look_at(cams[i], np.array([0.0, 2.5, 0.0]))
        Rs.append(R); ts.append(-R @ cams[i])
    n = len(obs_sets)
    u = rng.uniform(3 * n).reshape(n, 3)
    pts = np.stack([(u[:, 0] - 0.5) * 1.6, 1.8 + u[:, 1] * 1.6, (u[:, 2] - 0.5) * 1.0], 1)
    width = max(len(s) for s in obs_sets)
    cand = np.full((n, width), -1, np.int64)
    for q, s in enumerate(obs_sets):
        assert len(set(int(v) for v in s)) == len(s) >= 2
        cand[q, :len(s)] = s
    g = synth._finish_graph(rng, Rs, ts, pts, cand, fixed_mask(n_free, n_fixed), width, True,
                            rot_sigma=sigma[0], trans_sigma=sigma[1], pt_sigma=sigma[2])
    assert len(g["points"]) == n, "a landmark left an image"
    return g


def edge_counts(g):
    """Per landmark: edges on free keyframes, edges in all."""
    L = len(g["points"])
    free = g["fixed"][g["edge_pose"]] == 0
    return np.bincount(g["edge_point"][free], minlength=L), np.bincount(g["edge_point"], minlength=L)


def reordered(g, order):
    return dict(g, edge_pose=g["edge_pose"][order], edge_point=g["edge_point"][order], obs=g["obs"][order], info=g["info"][order])


def reversed_edges(g):
    return reordered(g, np.arange(len(g["edge_pose"]))[::-1])


def _spread_sets(P, n, rng, keyframes=None):
    """n landmarks of 6 observations spread over the arc (fewer where there are fewer than 6 keyframes)."""
    kfs = np.arange(P) if keyframes is None else np.asarray(keyframes)
    m = len(kfs)
    return [kfs[np.unique((a + np.arange(6) * max(1, m // 7)) % m)] for a in rng.integers(0, m, n)]


def _n_landmarks(P):
    return max(120, 6 * P)


def d_graph(nfree, variant="spread", n_fixed=2, seed=None):
    """D.  spread: landmarks of 6 observations spread over the arc.  full: the same, and more until every pair of keyframes shares a
    landmark.  band: every landmark seen by 6 consecutive keyframes, so only neighbours share one.  isolated: one free keyframe
    (the middle one) has no edge at all."""
    P = nfree + n_fixed
    rng = np.random.default_rng(1000 + nfree)
    n = _n_landmarks(P)
    if variant == "spread":
        sets = _spread_sets(P, n, rng)
    elif variant == "full":
        sets = _spread_sets(P, n, rng)
        seen = np.zeros((P, P), bool)
        for s in sets:
            seen[np.ix_(s, s)] = True
        for i in range(P):
            for j in range(i + 1, P):
                if not seen[i, j]:
                    rest = np.setdiff1d(np.arange(P), [i, j])
                    s = np.sort(np.concatenate([[i, j], rng.choice(rest, 4, replace=False)]))
                    sets.append(s); seen[np.ix_(s, s)] = True
    elif variant == "band":
        sets = [np.arange(a, a + 6) for a in np.arange(n) % (P - 5)]
    elif variant == "isolated":
        sets = _spread_sets(P, n, rng, np.delete(np.arange(P), isolated_keyframe(nfree, n_fixed)))
    else:
        raise ValueError(variant)
    return graph(nfree, n_fixed, sets, nfree if seed is None else seed)


def isolated_keyframe(nfree, n_fixed=2):
    return int(np.flatnonzero(~fixed_mask(nfree, n_fixed))[nfree // 2])


# L: (free edges, fixed edges) per landmark of the 60 + 4 graph, in the order the landmarks take (then repeated): the long lists
# alternate with short ones, so a landmark that takes the row form of the pair enumeration has neighbours in its workgroup that
# enumerate from LDS
L_ROWS = ((0, 2), (0, 4), (1, 1), (2, 0), (7, 0), (8, 0), (9, 0), (15, 0), (16, 0), (17, 0), (47, 0), (49, 0), (48, 0), (56, 0), (48, 4), (60, 0))
L_REPEAT = 5               # 80 landmarks: two full workgroups of 32 and a part of a third


def l_graph(seed=60):
    fixed = fixed_mask(60, 4)
    free_kf, fixed_kf = np.flatnonzero(~fixed), np.flatnonzero(fixed)
    rng = np.random.default_rng(2060)
    sets = []
    for _ in range(L_REPEAT):
        for k, f in L_ROWS:
            sets.append(np.sort(np.concatenate([rng.choice(free_kf, k, replace=False), rng.choice(fixed_kf, f, replace=False)])))
    return graph(60, 4, sets, seed)


def l_landmarks_graph(n_landmarks):
    """3 free + 2 fixed keyframes, every landmark seen by 4 of the 5: 31 / 32 / 33 landmarks fill a workgroup of the landmark kernels
    but for one, exactly, and start a second."""
    return graph(3, 2, [np.delete(np.arange(5), q % 5) for q in range(n_landmarks)], 100 + n_landmarks)


def l_edges_graph(n_edges):
    """6 free + 2 fixed keyframes and exactly n_edges edges (255 / 256 / 257: the 256-thread stride of the edge kernels)."""
    sizes = [5] * 49 + {255: [5, 5], 256: [5, 6], 257: [6, 6]}[n_edges]
    assert sum(sizes) == n_edges
    return graph(6, 2, [np.sort((q + np.arange(k)) % 8) for q, k in enumerate(sizes)], 200 + n_edges)


def s_graph(nfree, seed=None):
    """S.  Every edge of landmark 0 and of one free keyframe moved by 60-200 px: after the first stage of the local schedule all of
    them are outliers, and the second stage sees an all-zero Hll block and an all-zero Hpp block."""
    P = nfree + 2
    rng = np.random.default_rng(3000 + nfree)
    free_kf = np.flatnonzero(~fixed_mask(nfree, 2))
    sets = [np.sort(rng.choice(P, 5, replace=False)) for _ in range(_n_landmarks(P))]
    g = graph(nfree, 2, sets, (500 + nfree) if seed is None else seed)
    kf = stranded_keyframe(nfree)
    assert kf in free_kf
    moved = (g["edge_point"] == 0) | (g["edge_pose"] == kf)
    shift = rng.uniform(60, 200, (int(moved.sum()), 2)) * rng.choice([-1.0, 1.0], (int(moved.sum()), 2))
    obs = g["obs"].copy()
    obs[moved] = (obs[moved] + shift).astype(np.float32).astype(np.float64)          # keypoints are float32
    return dict(g, obs=obs, moved=moved)


def stranded_keyframe(nfree):
    return int(np.flatnonzero(~fixed_mask(nfree, 2))[3])


# ------------------------------------------------------------------------------------------------------------ the committed cases
# name -> (builder, arguments).  D: solver size; L: list lengths; S: inactive edges; P: graphs for the forced PCG.
D_SMALL = {"D1": (1, "spread"), "D2": (2, "spread"), "D22": (22, "spread"),
           "D23-full": (23, "full"), "D23-band": (23, "band"), "D23-isolated": (23, "isolated"),
           "D24-full": (24, "full"), "D24-band": (24, "band"), "D24-isolated": (24, "isolated"), "D25": (25, "spread")}
D_LARGE = {"D255": (255, "spread"), "D256": (256, "spread"), "D257": (257, "spread")}
D_ONE_FIXED = {"D23-one-fixed": (23, "spread", 1), "D257-one-fixed": (257, "spread", 1)}      # like MapFusionGBA: oracle only
L_CASES = {"L60": (l_graph,), "L-31-landmarks": (l_landmarks_graph, 31), "L-32-landmarks": (l_landmarks_graph, 32),
           "L-33-landmarks": (l_landmarks_graph, 33), "L-255-edges": (l_edges_graph, 255), "L-256-edges": (l_edges_graph, 256),
           "L-257-edges": (l_edges_graph, 257)}
S_CASES = {"S10": (s_graph, 10), "S30": (s_graph, 30)}
P_SIZES = (1, 7, 8, 9, 17, 31, 32, 33, 144, 145, 161)
P_CASES = {"P%d" % n: (n, "spread") for n in P_SIZES}

# name -> seed of `graph` where the default seed failed a condition of test_ba_cases_cpu.py
# (S10: with seeds 510, 511 and 512 the oracle kept one of the stranded keyframe's 59 moved edges as an inlier)
RESEEDED = {"S10": 513}

ONE_STEP_CASES = tuple(D_SMALL) + tuple(L_CASES) + tuple(S_CASES)            # the cases held to one_step
FULL_CASES = tuple(D_SMALL) + tuple(D_LARGE) + tuple(D_ONE_FIXED) + tuple(L_CASES) + tuple(S_CASES)
ALL_CASES = FULL_CASES + tuple(P_CASES)

_GRAPHS = {}


def case(name):
    """The graph of a committed case (built once per process; treat it as read-only)."""
    if name not in _GRAPHS:
        kw = {"seed": RESEEDED[name]} if name in RESEEDED else {}
        for table in (D_SMALL, D_LARGE, D_ONE_FIXED, P_CASES):
            if name in table:
                _GRAPHS[name] = d_graph(*table[name], **kw)
        for table in (L_CASES, S_CASES):
            if name in table:
                _GRAPHS[name] = table[name][0](*table[name][1:], **kw)
    return _GRAPHS[name]


# the full schedules every case runs: (label, iterations, huber, iterations2)
SCHEDULES = (("global3", 3, HUBER_GLOBAL, 0), ("local", 5, HUBER_LOCAL, 10))


# ------------------------------------------------------------------------------------------------------------ one LM iteration
def quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def pose_Rt(poses):
    """pose7 rows (qx, qy, qz, qw, t) as rotation matrices and translations."""
    poses = np.asarray(poses, np.float64)
    return np.stack([quat_R(p[:4] / np.linalg.norm(p[:4])) for p in poses]), poses[:, 4:7].copy()


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def se3_exp(d):
    """SE3Quat::exp (se3quat.h:223-257): d = (omega, upsilon) -> R, t, with its own small-angle branch."""
    w, v = d[:3], d[3:]
    th = np.linalg.norm(w)
    Om = skew(w)
    if th < 0.00001:
        R = np.eye(3) + Om + Om @ Om
        V = R
    else:
        R = np.eye(3) + np.sin(th) / th * Om + (1 - np.cos(th)) / th ** 2 * (Om @ Om)
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * Om + (th - np.sin(th)) / th ** 3 * (Om @ Om)
    return R, V @ v


def residuals(g, R, t, X):
    """obs - projection per edge [E, 2], and the camera-frame points [E, 3] (EdgeSE3ProjectXYZ::computeError)."""
    ep, el = g["edge_pose"], g["edge_point"]
    Xc = np.einsum("eij,ej->ei", R[ep], X[el]) + t[ep]
    fx, fy, cx, cy = g["intr"][ep].T
    proj = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    return g["obs"] - proj, Xc


def jacobians(g, R, Xc):
    """d error / d pose increment [E, 2, 6] (rotation first) and d error / d point [E, 2, 3] (types_six_dof_expmap.cpp:103-139)."""
    ep = g["edge_pose"]
    fx, fy = g["intr"][ep, 0], g["intr"][ep, 1]
    x, y, z = Xc.T
    o = np.zeros_like(x)
    Jp = np.stack([np.stack([x * y / z ** 2 * fx, -(1 + x * x / z ** 2) * fx, y / z * fx, -fx / z, o, x / z ** 2 * fx], 1),
                   np.stack([(1 + y * y / z ** 2) * fy, -x * y / z ** 2 * fy, -x / z * fy, o, -fy / z, y / z ** 2 * fy], 1)], 1)
    tmp = np.stack([np.stack([fx, o, -x / z * fx], 1), np.stack([o, fy, -y / z * fy], 1)], 1)
    Jl = np.einsum("eij,ejk->eik", -tmp / z[:, None, None], R[ep])
    return Jp, Jl


def robust_chi2(g, err, huber):
    """activeRobustChi2: sum of rho(info |err|^2), rho the Huber kernel of width huber (identity for huber = 0)."""
    c2 = g["info"] * (err ** 2).sum(1)
    if huber > 0:
        c2 = np.where(c2 <= huber * huber, c2, 2 * np.sqrt(c2) * huber - huber * huber)
    return float(c2.sum())


def one_step(g, huber):
    """One Levenberg iteration of g2o on the whole graph in float64 numpy: the full normal equations of keyframes and landmarks
    (no Schur complement) with the Huber weight rho' on information and right-hand side, lambda = 1e-5 max diag H
    (optimization_algorithm_levenberg.cpp:166-180), a dense solve, pose <- exp(delta) pose, point <- point + delta; a trial that
    does not lower the robust chi2 is taken back and repeated with lambda times 2, 4, 8 ... (:102-149), an accepted one scales
    lambda by 1 - (2 rho - 1)^3 cropped to [1/3, 2/3].  Returns R [P, 3, 3], t [P, 3], points [L, 3], lam (the first lambda),
    lam_final and trials.  huber = 0: no kernel."""
    R, t = pose_Rt(g["poses"])
    X = np.asarray(g["points"], np.float64)
    free = np.flatnonzero(g["fixed"] == 0)
    F, L = len(free), len(X)
    col = -np.ones(len(R), int); col[free] = 6 * np.arange(F)
    err, Xc = residuals(g, R, t, X)
    Jp, Jl = jacobians(g, R, Xc)
    n = 6 * F + 3 * L
    H = np.zeros((n, n)); b = np.zeros(n)
    for e in range(len(err)):
        om = g["info"][e]
        c2 = om * (err[e] @ err[e])
        w = om if (huber <= 0 or c2 <= huber * huber) else om * huber / np.sqrt(c2)
        il = 6 * F + 3 * g["edge_point"][e] + np.arange(3)
        if col[g["edge_pose"][e]] >= 0:
            idx = np.concatenate([col[g["edge_pose"][e]] + np.arange(6), il]); J = np.concatenate([Jp[e], Jl[e]], 1)
        else:
            idx = il; J = Jl[e]
        H[np.ix_(idx, idx)] += w * (J.T @ J)
        b[idx] -= w * (J.T @ err[e])
    chi = robust_chi2(g, err, huber)
    lam0 = lam = 1e-5 * np.abs(np.diag(H)).max()
    ni = 2.0
    for trial in range(1, 11):                                       # _maxTrialsAfterFailure is 10
        d = np.linalg.solve(H + lam * np.eye(n), b)
        R1, t1 = R.copy(), t.copy()
        for k, p in enumerate(free):
            dR, dt = se3_exp(d[6 * k:6 * k + 6])
            R1[p] = dR @ R[p]; t1[p] = dR @ t[p] + dt
        X1 = X + d[6 * F:].reshape(L, 3)
        rho = (chi - robust_chi2(g, residuals(g, R1, t1, X1)[0], huber)) / (d @ (lam * d + b) + 1e-3)
        if rho > 0 and np.isfinite(rho):
            lam *= max(1.0 / 3.0, min(2.0 / 3.0, 1.0 - (2 * rho - 1) ** 3))
            return dict(R=R1, t=t1, points=X1, lam=lam0, lam_final=lam, trials=trial, rho=rho)
        lam *= ni; ni *= 2
    raise ValueError("no trial of the iteration was accepted")


def structure_counts(g):
    """schur_pairs = sum of k (k + 1) / 2 over the landmarks, k = edges on free keyframes; schur_blocks = distinct pairs a <= b of
    free keyframes that share a landmark, plus the diagonal block of every free keyframe."""
    free = np.flatnonzero(g["fixed"] == 0)
    F, L = len(free), len(g["points"])
    k, _ = edge_counts(g)
    col = -np.ones(len(g["fixed"]), int); col[free] = np.arange(F)
    on_free = col[g["edge_pose"]] >= 0
    A = np.zeros((L, F))
    A[g["edge_point"][on_free], col[g["edge_pose"][on_free]]] = 1
    share = (A.T @ A) > 0
    return dict(schur_pairs=int((k * (k + 1) // 2).sum()), schur_blocks=F + int(np.triu(share, 1).sum()))


# ------------------------------------------------------------------------------------------------------------ tolerances
ORDER_TOL = 1e-10          # admissibility: the oracle under a reversed edge list and between its two solvers (optimizer_cases.py)
DEVICE_MARGIN = 1000.0     # over the reference's own sensitivity: the device's sqrt / division / sincos sequences (optimizer_cases.py)
FLOOR = 1e-12
CHI2_RTOL, CHI2_INITIAL_RTOL = 1e-9, 1e-10                 # test_ba_gpu.py
DENSE_POSE_CAP, DENSE_POINT_CAP = 1e-5, 1e-6               # test_ba_gpu.py: the dense path has never been allowed more
PCG_EXACT_CAP = 1e-9                                       # test_iterative_solver_forced_on_small_graphs at pcg_tol 1e-13
PCG_DEFAULT_POSE, PCG_DEFAULT_POINT = 1e-5, 1e-5           # test_ba_gpu.py: default pcg_tol, inexact by design
LAMBDA_CAP = 1e-6                                          # test_ba_gpu.py


ONE_STEP_ORACLE_TOL = 1e-12    # oracle's first iteration against one_step: two float64 evaluations (Schur complement / full system); 4.5e-14 measured

# name -> the reference's own sensitivity, measured on the CPU (rounded up to two digits; test_ba_cases_cpu.py asserts that what it
# measures stays within them and prints the figures):
#   [0] one_step: largest change of R, t, X under a reversed edge list (robust and not); 0 where the case has no one_step
#   [1] oracle, 3 global iterations: the larger change of pose7 / points under a reversed edge list and between its two solvers
#   [2] the same for the local schedule 5 + 10
#   [3] oracle: largest relative change of lambda_final under the same two changes, either schedule (where an accepted step's
#       factor 1 - (2 rho - 1)^3 is not cropped to 1/3, lambda follows rho: 1e-9 instead of 1e-16)
# Every entry is far below ORDER_TOL, so each case enters its checks.
SENS = {
    "D1": (3.1e-14, 1.8e-15, 1.8e-15, 4.5e-16),
    "D2": (9.5e-15, 1.8e-15, 1.8e-15, 1.2e-15),
    "D22": (1.4e-14, 5.4e-13, 6.6e-13, 5.6e-16),
    "D23-full": (2.3e-14, 2.9e-14, 4.0e-15, 2.3e-16),
    "D23-band": (2.9e-14, 4.7e-13, 8.6e-13, 2.3e-16),
    "D23-isolated": (1.8e-14, 5.0e-13, 9.4e-13, 1.9e-10),
    "D24-full": (1.6e-14, 1.7e-14, 3.6e-15, 2.3e-16),
    "D24-band": (3.3e-14, 1.3e-13, 1.1e-12, 0.0),
    "D24-isolated": (3.3e-14, 6.6e-13, 7.7e-14, 5.2e-11),
    "D25": (4.0e-14, 5.4e-13, 9.8e-13, 6.2e-11),
    "D255": (0.0, 4.1e-13, 2.6e-13, 2.3e-16),
    "D256": (0.0, 3.7e-13, 1.2e-12, 0.0),
    "D257": (0.0, 7.6e-13, 1.7e-12, 2.3e-16),
    "D23-one-fixed": (0.0, 5.6e-13, 2.2e-12, 2.3e-16),
    "D257-one-fixed": (0.0, 2.8e-13, 1.8e-12, 2.3e-16),
    "L60": (3.5e-14, 8.5e-14, 2.6e-14, 2.3e-16),
    "L-31-landmarks": (1.6e-14, 2.5e-15, 2.7e-15, 2.3e-16),
    "L-32-landmarks": (1.9e-14, 3.2e-15, 2.7e-15, 3.4e-16),
    "L-33-landmarks": (2.1e-14, 7.9e-15, 3.2e-15, 0.0),
    "L-255-edges": (3.1e-14, 2.7e-15, 2.7e-15, 3.4e-16),
    "L-256-edges": (7.4e-15, 3.2e-15, 2.7e-15, 4.5e-16),
    "L-257-edges": (9.4e-15, 4.5e-15, 3.2e-15, 2.3e-16),
    "S10": (1.7e-13, 8.1e-14, 6.5e-14, 2.3e-16),
    "S30": (4.1e-14, 2.3e-13, 1.4e-11, 9.6e-11),
    "P1": (0.0, 1.8e-15, 1.8e-15, 4.5e-16),
    "P7": (0.0, 2.7e-15, 2.7e-15, 4.5e-16),
    "P8": (0.0, 4.0e-15, 9.1e-14, 2.4e-09),
    "P9": (0.0, 3.6e-15, 3.2e-15, 4.5e-16),
    "P17": (0.0, 7.6e-14, 9.5e-15, 6.7e-16),
    "P31": (0.0, 1.4e-13, 1.1e-13, 4.5e-16),
    "P32": (0.0, 7.6e-13, 5.8e-13, 2.1e-11),
    "P33": (0.0, 2.9e-13, 9.5e-13, 4.5e-16),
    "P144": (0.0, 2.5e-13, 1.0e-12, 4.5e-16),
    "P145": (0.0, 3.3e-13, 1.7e-12, 4.5e-16),
    "P161": (0.0, 4.5e-13, 6.1e-13, 4.5e-16),
}


def bound(s, cap):
    """What a device result may differ by from a reference of sensitivity s: max(1e-12, 1000 s), never looser than the bound `cap`
    the suite already holds that path to."""
    return min(max(FLOOR, DEVICE_MARGIN * s), cap)
