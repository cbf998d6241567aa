"""Pose-only problems of a chosen size for the optimiser tests: one frame, n correspondences, every quantity rounded the way the
tracker hands it over (map-point positions and keypoints through float32, invSigma2 as float).  Unlike synth.local_ba_graph this
gives a one-frame problem of exactly n edges, so the tests can sit on the 64-lane wave, the 256-thread stride and the n < 10 /
n < 3 rules of Optimizer::PoseOptimizationClient (src/Optimizer.cpp:215-347).  tests/test_optimizer_cases_cpu.py checks on the
CPU oracle that every case listed here reaches the branch it is meant for; tests/test_pose_gpu.py runs them on the GPU.
Further down: the frames of the handle-form tests (test_frame_gpu.py, test_search_local_points_gpu.py) and the Sim3, essential-graph
and map-point-correction cases of test_sim3_gpu.py.  A plain module: no fixtures, nothing that needs a GPU."""
import numpy as np

from sim3_problems import make_problem, rand_sim3  # noqa: F401  (rand_sim3: used by the tests through this module)

K = np.array([458.654, 457.296, 367.215, 248.375])

# pose tolerance of the GPU tests against the oracle (max |pose7 - oracle pose7|): three orders above the oracle's own
# sensitivity to the edge order (test_optimizer_cases_cpu.py holds that to 1e-10), left for the device's sqrt / pow / sin / cos
POSE_TOL = 1e-8
ORDER_TOL = 1e-10          # oracle forward vs reversed edge order
ORDER_TOL_FAR = 1e-8       # the same for the far-start case (more iterations, larger steps)


def quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def project(pose, pts):
    """Pixel coordinates and camera-frame depth of world points under pose7 = qx,qy,qz,qw,tx,ty,tz (float64)."""
    pc = np.asarray(pts, np.float64) @ quat_R(pose[:4]).T + pose[4:7]
    return np.stack([pc[:, 0] / pc[:, 2] * K[0] + K[2], pc[:, 1] / pc[:, 2] * K[1] + K[3]], 1), pc[:, 2]


def chi2(pose, pts, obs, info, mask=None):
    """Sum of info * |obs - projection|^2 over the edges of mask, in float64 numpy: independent of kernel and oracle."""
    uv, _ = project(np.asarray(pose, np.float64), pts)
    c = np.asarray(info, np.float64) * ((np.asarray(obs, np.float64) - uv) ** 2).sum(1)
    return float(c.sum() if mask is None else c[np.asarray(mask, bool)].sum())


def camera_points(rng, n):
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2.5, 9, n)], 1)


def world_points(gt, cam):
    """Camera-frame points moved to the world frame of pose gt and rounded through float32 (MapPoint positions are float32)."""
    return f32((np.asarray(cam, np.float64) - gt[4:7]) @ quat_R(gt[:4]))          # Xw = R^T (Xc - t)


def pose_case(seed, n, noise=0.5, start=0.03):
    """gt pose, n points seen from it, noisy observations and a perturbed start pose."""
    rng = np.random.default_rng(seed)
    q = np.concatenate([rng.normal(0, 0.05, 3), [1.0]]); q /= np.linalg.norm(q)
    gt = np.concatenate([q, rng.normal(0, 0.5, 3)])
    pc = camera_points(rng, n)
    lvl = rng.integers(0, 8, n)
    pix = rng.normal(0, 1, (n, 2))
    dq = rng.normal(0, start * 0.3, 4); dt = rng.normal(0, start, 3)
    pts = world_points(gt, pc)
    uv, _ = project(gt, pts)
    obs = f32(uv + noise * (1.2 ** lvl)[:, None] * pix)               # keypoints are float32
    info = f32(1.0 / 1.2 ** (2 * lvl))                                # mvInvLevelSigma2 is float
    start_pose = gt.copy()
    start_pose[:4] += dq; start_pose[:4] /= np.linalg.norm(start_pose[:4]); start_pose[4:] += dt
    return dict(pose=start_pose, intr=K.copy(), pts=pts, obs=obs, info=info, gt=gt, n=n, level=lvl.astype("i4"))


def with_wrong_matches(obs, rng, every=7, sigma=30):
    """Every `every`-th observation moved by N(0, sigma) pixels: a wrong match."""
    obs = obs.copy()
    obs[::every] = f32(obs[::every] + rng.normal(0, sigma, obs[::every].shape))
    return obs


# ------------------------------------------------------------------------------------------------------------ the committed cases
SIZES_A = (3, 4, 9, 10, 11, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
# case A on the CPU oracle, seed = n: n -> inliers (test_optimizer_cases_cpu.py asserts these)
INLIERS_A = {3: 3, 4: 4, 9: 7, 10: 8, 11: 9, 63: 54, 64: 54, 65: 55, 255: 218, 256: 220, 257: 220, 511: 439, 512: 439, 513: 440, 1025: 880}
# n -> seed of the wrong matches where 1000 + n failed a condition of test_optimizer_cases_cpu.py
# (513: the oracle's pose moved 1.4e-10 under a reversed edge order, above ORDER_TOL)
WRONG_SEED_A = {513: 2002}


def case_a(n):
    """A. one frame of n correspondences, every 7th a wrong match; seed = n."""
    c = pose_case(n, n)
    c["obs"] = with_wrong_matches(c["obs"], np.random.default_rng(WRONG_SEED_A.get(n, 1000 + n)))
    return c


def case_two():
    """Fewer than 3 correspondences: returns 0, pose untouched."""
    return pose_case(2, 2)


def case_c():
    """C. 200 correspondences, every observation 40-200 px off with a random sign: all outliers after round 0."""
    c = pose_case(200, 200)
    rng = np.random.default_rng(1200)
    c["obs"] = f32(c["obs"] + rng.uniform(40, 200, c["obs"].shape) * rng.choice([-1.0, 1.0], c["obs"].shape))
    return c


BEHIND_D = (7, 23, 41, 66, 90)


def case_d():
    """D. 100 correspondences; the map points of 5 of them lie behind the camera (camera-frame z about -3, never 0: NaN is not
    part of the contract) while their keypoints stay where they were -- wrong matches with a negative depth."""
    c = pose_case(100, 100)
    rng = np.random.default_rng(1300)
    idx = list(BEHIND_D)
    cam = camera_points(rng, len(idx))
    cam[:, 2] = -3 + rng.uniform(-0.2, 0.2, len(idx))
    c["pts"][idx] = world_points(c["gt"], cam)
    return c


def case_e_rank():
    """E1. 50 copies of one correspondence: H has rank 2, only lambda makes it positive definite."""
    c = pose_case(50, 1)
    return dict(c, pts=np.repeat(c["pts"], 50, 0), obs=np.repeat(c["obs"], 50, 0), info=np.repeat(c["info"], 50), n=50)


def case_e_far():
    """E2. a clean 300-point frame started far away (start = 0.3)."""
    return pose_case(300, 300, start=0.3)


def reversed_case(c):
    return dict(c, pts=c["pts"][::-1].copy(), obs=c["obs"][::-1].copy(), info=c["info"][::-1].copy())


def batch(cases):
    """Concatenate one-frame cases into the arrays of Optimizer.PoseOptimizationClient."""
    first = np.concatenate([[0], np.cumsum([len(c["info"]) for c in cases])]).astype("i4")
    cat = lambda k, w: np.concatenate([np.asarray(c[k], "f8").reshape(-1, w) for c in cases]) if w else np.concatenate([c[k] for c in cases])
    return (np.stack([c["pose"] for c in cases]), np.stack([c["intr"] for c in cases]), first, cat("pts", 3), cat("obs", 2), cat("info", 0))


def empty_case(seed):
    c = pose_case(seed, 3)
    return dict(c, pts=c["pts"][:0], obs=c["obs"][:0], info=c["info"][:0], n=0)


# ------------------------------------------------------------------------------------------------------------ frames (handle forms)
FRAME_SIZES = (1023, 1024, 1025, 2049)
FRAME_PATTERNS = ("all", "last", "lanes0", "alternate", "three")
FRAME_BOUNDS = (-300.0, 1100.0, -300.0, 800.0)      # mnMinX, mnMaxX, mnMinY, mnMaxY wide enough for every keypoint of pose_case


def frame_mask(N, pattern):
    """Which features of an N-feature frame carry a map point: the edges of the single-workgroup compaction (1024 threads, one
    ballot per 64-lane wave, a running base per 1024-block)."""
    i = np.arange(N)
    if pattern == "all":
        return np.ones(N, bool)
    if pattern == "last":                                          # only the last feature plus two others
        return (i == N - 1) | (i == 0) | (i == N // 2)
    if pattern == "lanes0":                                        # wave 0 of every 1024-block empty
        return (i % 1024) >= 64
    if pattern == "alternate":                                     # every second 64-group empty
        return (i // 64) % 2 == 1
    if pattern == "three":                                         # exactly 3, none of them first or last
        return (i == 5) | (i == N // 3) | (i == N - 2)
    raise ValueError(pattern)


def frame_case(N, pattern):
    """An N-feature frame for the handle forms of PoseOptimizationClient: keypoints kx / ky / oct, mp_id per feature (-1 = none,
    else a row of `table`, whose order differs from the feature order), the start pose and the intrinsics.  Features with a map
    point observe it (every 7th wrongly); the others lie anywhere."""
    c = pose_case(N, N)
    obs = with_wrong_matches(c["obs"], np.random.default_rng(3000 + N))
    rng = np.random.default_rng(4000 + N)
    mask = frame_mask(N, pattern)
    row = rng.permutation(N)                                       # feature i's map point is table row row[i]
    table = np.zeros((N, 3)); table[row] = c["pts"]
    kx = np.where(mask, obs[:, 0], rng.uniform(0, 752, N)).astype("f4"); ky = np.where(mask, obs[:, 1], rng.uniform(0, 480, N)).astype("f4")
    ids = np.where(mask, row, -1).astype("i4")
    return dict(kx=kx, ky=ky, oct=c["level"], ids=ids, table=table, pose=c["pose"], intr=c["intr"], mask=mask, gt=c["gt"])


def gathered(fc, is2):
    """The array problem the handle forms must reproduce: the features with a map point, in feature order."""
    m = fc["mask"]
    return (fc["table"][fc["ids"][m]], np.stack([fc["kx"][m], fc["ky"][m]], 1).astype("f8"), np.asarray(is2, "f4")[fc["oct"][m]].astype("f8"))


# ------------------------------------------------------------------------------------------------------------ Sim3, essential graph
def sim3_survivor_problem(nb):
    """12 clean pairs of which the first nb are pushed 40 px away: 12 - nb survive the first round of OptimizeSim3, so nb = 2
    sits exactly on the reference's "fewer than 10 left -> return 0" rule (src/Optimizer.cpp:1022-1023) and nb = 3 just below."""
    p = make_problem(np.random.default_rng(50 + nb), 12, outlier_frac=0, noise=0.3, start_err=0.02)
    p["obs1"][:nb] += 40
    return p


SIM3_SURVIVOR_NB = (1, 2, 3, 4)
SIM3_SURVIVOR_TH2 = (10.0, 20.0, 10.0, 20.0)
SIM3_SURVIVOR_INLIERS = (11, 10, 0, 0)


# seed of make_pose_graph(n=40) for the essential-graph cases.  The reference takes the Jacobians numerically (delta 1e-9), which
# turns a last-bit difference of an error into 1e-7 of a Jacobian entry; on graphs where Levenberg stalls for many iterations that
# decides where it stops (seed 140 with vertices 0 and 20 fixed: the oracle's dense and block-sparse solvers end 3e-5 apart, seed 149
# 1.5 apart).  test_optimizer_cases_cpu.py holds every case built from this seed to ESS_COND between the oracle's two solvers and
# under a one-ulp change of the input, one order below the 1e-6 the GPU is held to.
ESS_SEED = 147
ESS_COND = 1e-7


def relabel_graph(perm, sim3, fixed, ei, ej):
    """Vertex v becomes vertex perm[v]."""
    s = np.empty_like(sim3); s[perm] = sim3
    f = np.empty_like(fixed); f[perm] = fixed
    return s, f, perm[ei].astype("i4"), perm[ej].astype("i4")


def swap_edges(oracle, ei, ej, meas):
    """Every edge written the other way round (vertex 0 < vertex 1): Sij = Sji^-1."""
    return ej.copy(), ei.copy(), np.array([oracle.sim3_inverse(m) for m in meas])


def two_chain_graph(oracle, sim3, ei, ej, meas, truth, mid):
    """Vertex `mid` fixed and only the edges that do not pass over it, so the free vertices form two components that share no block
    of H; each side gets a loop edge to `mid` measured from the truth, like the loop edge of make_pose_graph, so that its optimum is
    a compromise with the drifted chain and not a zero residual."""
    n = len(sim3)
    keep = ~(((ei > mid) & (ej < mid)) | ((ej > mid) & (ei < mid)))
    ci, cj, cm = list(ei[keep]), list(ej[keep]), list(meas[keep])
    for i, j in ((n - 1, mid), (mid, 0)):
        ci.append(i); cj.append(j); cm.append(oracle.sim3_mul(truth[j], oracle.sim3_inverse(truth[i])))
    fixed = np.zeros(n, np.uint8); fixed[mid] = 1
    return fixed, np.array(ci, "i4"), np.array(cj, "i4"), np.array(cm)


def two_vertex_graph():
    """Vertex 0 fixed, one edge 1 -> 0 whose residual is exactly zero: identity rotation and unit scale make every product exact."""
    s = np.array([[0, 0, 0, 1, 0, 0, 0, 1.0], [0, 0, 0, 1, 0.5, -0.25, 1.0, 1.0]])
    meas = np.array([[0, 0, 0, 1, -0.5, 0.25, -1.0, 1.0]])                          # S0 * S1^-1
    return s, np.array([1, 0], np.uint8), np.array([1], "i4"), np.array([0], "i4"), meas


def sim3_apply(S, X):
    """S.map(X) per row in float64 numpy: s R X + t."""
    return S[:, 7:8] * np.einsum("nij,nj->ni", np.stack([quat_R(q) for q in S[:, :4]]), X) + S[:, 4:7]


def sim3_inv(S):
    """Sim3::inverse per row in float64 numpy (sim3.h:245-248)."""
    out = S.copy()
    out[:, :3] = -S[:, :3]
    out[:, 7] = 1.0 / S[:, 7]
    Rt = np.stack([quat_R(q).T for q in S[:, :4]])
    out[:, 4:7] = -np.einsum("nij,nj->ni", Rt, S[:, 4:7]) / S[:, 7:8]
    return out


def correct_map_points_ref(points, ref_vertex, before, after):
    """inverse(after[r]) o before[r] applied to every point with r >= 0; the others stay (src/Optimizer.cpp:1300-1330)."""
    out = np.array(points, np.float64)
    m = np.asarray(ref_vertex) >= 0
    if not m.any():
        return out
    r = np.asarray(ref_vertex)[m]
    out[m] = sim3_apply(sim3_inv(after[r]), sim3_apply(before[r], out[m]))
    return out
