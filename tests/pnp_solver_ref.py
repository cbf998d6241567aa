"""A numpy float64 restatement of cslam::PnPsolver (src/PnPSolver.cpp), the definition the batched solver is held to.

EPnP depends on two arbitrary choices of the SVD the reference calls: the signs of the PCA axes (choose_control_points, :391) and
the basis of the null space of M^T M that compute_pose reads as "the four smallest right singular vectors" (:755-758; with four
correspondences that null space is 4-dimensional).  epnp() therefore takes the pair (control points, basis) as an input when the
caller has one (the library taps its own), and only falls back to numpy's eigh.  Everything behind the pair is well conditioned.
"""
import math

import numpy as np

PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]           # the (a, b) order of :763-774 and :795-800
AXIS_EPS, RANK_EPS = 1e-7, 1e-12                                    # pseudo-inverse and least-squares rank thresholds (relative)


# ------------------------------------------------------------------------------------------------ SetRansacParameters :119-142
def ransac_parameters(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """-> (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon as float32)"""
    eps = np.float32(epsilon)
    n_min = int(np.float32(n) * eps)                                # :124, int * float is a float product
    n_min = max(n_min, int(min_inliers), int(min_set))              # :125-128
    with np.errstate(all="ignore"):
        ratio = np.float32(n_min) / np.float32(n)                   # :131
    if eps < ratio:
        eps = ratio
    if n < n_min or n_min == n:                                     # n < n_min: undefined and unused in the reference, 1 here
        its = 1
    else:
        v = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3)))      # :140
        its = int(min(v, max_iterations))
    return n_min, max(1, min(its, int(max_iterations))), eps        # :142


# ------------------------------------------------------------------------------------------------------ sampling :178-192
def sample_indices(n, draws):
    avail = list(range(n)); out = []
    for r in draws:
        out.append(avail[r]); avail[r] = avail[-1]; avail.pop()
    return out


# -------------------------------------------------------------------------------------------------------------- EPnP :366-941
def control_points(pw):
    """choose_control_points :366-400 with numpy's eigh: cws [4][3]"""
    n = len(pw)
    c0 = pw.sum(0) / n
    w, v = np.linalg.eigh((pw - c0).T @ (pw - c0))
    w, v = w[::-1], v[:, ::-1]                                      # cvSVD orders descending
    return np.vstack([c0, c0 + np.sqrt(np.maximum(w, 0) / n)[:, None] * v.T])


def barycentric(pw, cws):
    """compute_barycentric_coordinates :402-425, cvInvert(CV_SVD) as a pseudo-inverse"""
    CC = (cws[1:] - cws[0]).T
    ci = np.linalg.pinv(CC, rcond=AXIS_EPS)
    a = np.empty((len(pw), 4))
    a[:, 1:] = (pw - cws[0]) @ ci.T
    a[:, 0] = 1.0 - a[:, 1] - a[:, 2] - a[:, 3]
    return a


def fill_M(alphas, us, K):
    """:427-442, :473-476: M [2n][12]"""
    fu, fv, uc, vc = K
    n = len(us)
    M = np.zeros((2 * n, 12))
    for i in range(4):
        M[0::2, 3 * i] = alphas[:, i] * fu; M[0::2, 3 * i + 2] = alphas[:, i] * (uc - us[:, 0])
        M[1::2, 3 * i + 1] = alphas[:, i] * fv; M[1::2, 3 * i + 2] = alphas[:, i] * (vc - us[:, 1])
    return M


def null_basis(M):
    """v[0..3] = ut rows 11..8 (:755-758) with numpy's eigh: the eigenvectors of the four smallest eigenvalues, smallest first"""
    w, v = np.linalg.eigh(M.T @ M)
    return v[:, :4].T.copy()


def L_6x10(v):
    """compute_L_6x10 :751-791"""
    L = np.empty((6, 10))
    for j, (a, b) in enumerate(PAIRS):
        dv = [v[i, 3 * a:3 * a + 3] - v[i, 3 * b:3 * b + 3] for i in range(4)]
        L[j] = [dv[0] @ dv[0], 2 * (dv[0] @ dv[1]), dv[1] @ dv[1], 2 * (dv[0] @ dv[2]), 2 * (dv[1] @ dv[2]), dv[2] @ dv[2],
                2 * (dv[0] @ dv[3]), 2 * (dv[1] @ dv[3]), 2 * (dv[2] @ dv[3]), dv[3] @ dv[3]]
    return L


def rho_of(cws):
    """compute_rho :793-801"""
    return np.array([((cws[a] - cws[b]) ** 2).sum() for a, b in PAIRS])


def _solve(A, b):
    return np.linalg.lstsq(A, b, rcond=RANK_EPS)[0]                 # cvSolve(CV_SVD): the minimum-norm least-squares solution


def betas_approx_1(L, rho):
    """:658-685"""
    b = _solve(L[:, [0, 1, 3, 6]], rho)
    s = -1.0 if b[0] < 0 else 1.0
    b0 = math.sqrt(s * b[0])
    return np.array([b0, s * b[1] / b0, s * b[2] / b0, s * b[3] / b0])


def _betas_01(b):
    if b[0] < 0:
        b0 = math.sqrt(-b[0]); b1 = math.sqrt(-b[2]) if b[2] < 0 else 0.0
    else:
        b0 = math.sqrt(b[0]); b1 = math.sqrt(b[2]) if b[2] > 0 else 0.0
    if b[1] < 0:
        b0 = -b0
    return b0, b1


def betas_approx_2(L, rho):
    """:690-717"""
    b0, b1 = _betas_01(_solve(L[:, [0, 1, 2]], rho))
    return np.array([b0, b1, 0.0, 0.0])


def betas_approx_3(L, rho):
    """:722-749"""
    b = _solve(L[:, [0, 1, 2, 3, 4]], rho)
    b0, b1 = _betas_01(b)
    return np.array([b0, b1, b[3] / b0, 0.0])


def qr_solve(A, b):
    """:851-941, in its operation order.  The scan for eta reads each entry before it advances, so it covers rows k .. nr-2.
    eta == 0: the reference returns with X stale; the step is zero here (the one deviation the library documents)."""
    A = A.copy(); b = b.copy()
    nr, nc = A.shape
    A1 = np.zeros(nc); A2 = np.zeros(nc)
    for k in range(nc):
        eta = abs(A[k, k])
        for i in range(k + 1, nr):
            eta = max(eta, abs(A[i - 1, k]))
        if eta == 0:
            return np.zeros(nc)
        inv_eta = 1.0 / eta
        s = 0.0
        for i in range(k, nr):
            A[i, k] *= inv_eta
            s += A[i, k] * A[i, k]
        sigma = math.sqrt(s)
        if A[k, k] < 0:
            sigma = -sigma
        A[k, k] += sigma
        A1[k] = sigma * A[k, k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = 0.0
            for i in range(k, nr):
                s += A[i, k] * A[i, j]
            tau = s / A1[k]
            for i in range(k, nr):
                A[i, j] -= tau * A[i, k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau += A[i, j] * b[i]
        tau /= A1[j]
        for i in range(j, nr):
            b[i] -= tau * A[i, j]
    x = np.zeros(nc)
    x[nc - 1] = b[nc - 1] / A2[nc - 1]
    for i in range(nc - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s += A[i, j] * x[j]
        x[i] = (b[i] - s) / A2[i]
    return x


def gauss_newton(L, rho, betas):
    """:803-849"""
    be = np.array(betas, "f8")
    for _ in range(5):
        A = np.empty((6, 4)); b = np.empty(6)
        for i in range(6):
            l = L[i]
            A[i, 0] = 2 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3]
            A[i, 1] = l[1] * be[0] + 2 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3]
            A[i, 2] = l[3] * be[0] + l[4] * be[1] + 2 * l[5] * be[2] + l[8] * be[3]
            A[i, 3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2 * l[9] * be[3]
            b[i] = rho[i] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] + l[4] * be[1] * be[2] +
                             l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] + l[8] * be[2] * be[3] + l[9] * be[3] * be[3])
        be = be + qr_solve(A, b)
    return be


def R_and_t(v, betas, alphas, pw, us, K):
    """compute_R_and_t :642-653 -> (R, t, reprojection error)"""
    ccs = (betas[:, None] * v).sum(0).reshape(4, 3)                 # compute_ccs :444-455
    pcs = alphas @ ccs                                              # compute_pcs :457-466
    if pcs[0, 2] < 0.0:                                             # solve_for_sign :627-640
        ccs, pcs = -ccs, -pcs
    n = len(pw)
    pc0 = pcs.sum(0) / n; pw0 = pw.sum(0) / n                       # estimate_R_and_t :560-618
    ABt = (pcs - pc0).T @ (pw - pw0)
    U, _, Vt = np.linalg.svd(ABt)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R[2] = -R[2]
    t = pc0 - R @ pw0
    P = pw @ R.T + t                                                # reprojection_error :541-558
    inv = 1.0 / P[:, 2]
    ue = K[2] + K[0] * P[:, 0] * inv; ve = K[3] + K[1] * P[:, 1] * inv
    return R, t, np.sqrt((us[:, 0] - ue) ** 2 + (us[:, 1] - ve) ** 2).sum() / n


def epnp(pw, us, K, cws=None, basis=None):
    """compute_pose :468-516 for correspondences pw [n][3], us [n][2] and K = fu, fv, uc, vc.  With cws and basis given, they
    replace choose_control_points' and the SVD's arbitrary choices."""
    pw = np.asarray(pw, "f8"); us = np.asarray(us, "f8"); K = np.asarray(K, "f8")
    with np.errstate(all="ignore"):
        cws = control_points(pw) if cws is None else np.asarray(cws, "f8")
        alphas = barycentric(pw, cws)
        v = null_basis(fill_M(alphas, us, K)) if basis is None else np.asarray(basis, "f8")
        L = L_6x10(v); rho = rho_of(cws)
        cands = []
        for approx in (betas_approx_1, betas_approx_2, betas_approx_3):
            be = gauss_newton(L, rho, approx(L, rho))
            cands.append((be,) + R_and_t(v, be, alphas, pw, us, K))
        N = 0                                                       # :509-511
        if cands[1][3] < cands[0][3]:
            N = 1
        if cands[2][3] < cands[N][3]:
            N = 2
    return dict(R=cands[N][1], t=cands[N][2], betas=cands[N][0], rep_error=np.array([c[3] for c in cands]), which=N + 1, cws=cws, basis=v,
                Rs=np.array([c[1] for c in cands]), ts=np.array([c[2] for c in cands]))


# ---------------------------------------------------------------------------------------------------- CheckInliers :299-330
def check_inliers(Rt, K, P3Dw, P2D, max_err):
    """Rt [..][12] float64 (R row-major, t), K float32 [4], P3Dw / P2D / max_err float32 -> flags [..][N], in the reference's types:
    Xc, Yc, invZc rounded to float32, ue / ve float64, the distances and error2 float32; a NaN error is an outlier."""
    Rt = np.asarray(Rt, "f8")[..., None, :]
    X, Y, Z = (np.asarray(P3Dw, "f4")[:, i].astype("f8") for i in range(3))
    u, v = (np.asarray(P2D, "f4")[:, i].astype("f8") for i in range(2))
    fu, fv, uc, vc = (float(x) for x in np.asarray(K, "f4"))
    f4 = np.float32
    with np.errstate(all="ignore"):
        Xc = (Rt[..., 0] * X + Rt[..., 1] * Y + Rt[..., 2] * Z + Rt[..., 9]).astype(f4)
        Yc = (Rt[..., 3] * X + Rt[..., 4] * Y + Rt[..., 5] * Z + Rt[..., 10]).astype(f4)
        invZc = (1 / (Rt[..., 6] * X + Rt[..., 7] * Y + Rt[..., 8] * Z + Rt[..., 11])).astype(f4)
        ue = uc + fu * Xc.astype("f8") * invZc.astype("f8")
        ve = vc + fv * Yc.astype("f8") * invZc.astype("f8")
        dX = (u - ue).astype(f4); dY = (v - ve).astype(f4)
        e2 = dX * dX + dY * dY
        return e2 < np.asarray(max_err, "f4")


def max_error(sigma2, th2=5.991):
    return np.asarray(sigma2, "f4") * np.float32(th2)               # :146


def tcw(Rt):
    T = np.eye(4, dtype="f4"); T[:3, :3] = np.asarray(Rt[:9], "f8").reshape(3, 3).astype("f4"); T[:3, 3] = np.asarray(Rt[9:], "f8").astype("f4")
    return T


# ------------------------------------------------------------------------------------------------------- iterate :155-249
class RefSolver:
    """PnPsolver::iterate / find / Refine over given per-hypothesis results, literally.  counts[h], masks[h] = mnInliersi, mvbInliersi
    of hypothesis h (in draw order); refine(mask) -> (count, mask) = mnRefinedInliers, mvbRefinedInliers of Refine() on
    mvbBestInliers = mask.  A returned pose is named, not computed: ("refined", h) = mRefinedTcw of the refinement of hypothesis h's
    mask, ("best", h) = mBestTcw of hypothesis h."""

    def __init__(self, N, n1, kp_index, counts, masks, min_inliers, max_its, refine):
        self.N, self.n1, self.kp_index = N, n1, kp_index
        self.counts, self.masks, self.refine = counts, masks, refine
        self.mRansacMinInliers, self.mRansacMaxIts = min_inliers, max_its
        self.mnIterations = 0; self.mnBestInliers = 0; self.best = -1

    def _vb(self, mask):
        vb = np.zeros(self.n1, bool)
        for i in range(self.N):
            if mask[i]:
                vb[self.kp_index[i]] = True
        return vb

    def iterate(self, nIterations):
        """-> (pose name or None, bNoMore, vbInliers, nInliers)"""
        bNoMore = False; vbInliers = np.zeros(self.n1, bool); nInliers = 0
        if self.N < self.mRansacMinInliers:
            return None, True, vbInliers, nInliers
        nCurrentIterations = 0
        while self.mnIterations < self.mRansacMaxIts or nCurrentIterations < nIterations:
            nCurrentIterations += 1
            h = self.mnIterations
            self.mnIterations += 1
            mnInliersi = self.counts[h]                             # IndexError here = beyond what was evaluated
            if mnInliersi >= self.mRansacMinInliers:
                if mnInliersi > self.mnBestInliers:
                    self.mvbBestInliers = self.masks[h]; self.mnBestInliers = mnInliersi; self.best = h
                mnRefinedInliers, mvbRefinedInliers = self.refine(self.mvbBestInliers)       # Refine() :251-296
                if mnRefinedInliers > self.mRansacMinInliers:
                    return ("refined", self.best), bNoMore, self._vb(mvbRefinedInliers), mnRefinedInliers
        if self.mnIterations >= self.mRansacMaxIts:
            bNoMore = True
            if self.mnBestInliers >= self.mRansacMinInliers:
                return ("best", self.best), bNoMore, self._vb(self.mvbBestInliers), self.mnBestInliers
        return None, bNoMore, vbInliers, nInliers

    def find(self):
        r = self.iterate(self.mRansacMaxIts)
        return r[0], r[2], r[3]


def records(counts, min_inliers):
    """The hypotheses that become the running best: count >= minInliers and > every earlier such count (mnBestInliers starts at 0)."""
    out = []; best = 0
    for h, c in enumerate(counts):
        if c >= min_inliers and c > best:
            best = c; out.append(h)
    return out


class ReplaySolver:
    """The library's replay rule (csrc/pnp_host.cpp), restated: one stored refinement per record, consulted by position.  ref_counts /
    ref_masks are in record order.  iterate returns "state" (CCM_E_STATE) and changes nothing when the call would read past n_hyp."""

    def __init__(self, N, n1, kp_index, counts, masks, min_inliers, max_its, ref_counts, ref_masks):
        self.N, self.n1, self.kp_index, self.counts, self.masks = N, n1, kp_index, counts, masks
        self.min_inliers, self.max_its, self.ref_counts, self.ref_masks = min_inliers, max_its, ref_counts, ref_masks
        self.rec = records(counts, min_inliers)
        self.iterations = 0; self.best_inliers = 0; self.best = -1; self.best_ref = -1

    _vb = RefSolver._vb

    def iterate(self, n_iterations):
        if self.N >= self.min_inliers and max(self.max_its, self.iterations + max(n_iterations, 0)) > len(self.counts):
            return "state"
        empty = np.zeros(self.n1, bool)
        if self.N < self.min_inliers:
            return None, True, empty, 0
        current = 0
        while self.iterations < self.max_its or current < n_iterations:
            current += 1
            h = self.iterations; self.iterations += 1
            c = self.counts[h]
            if c >= self.min_inliers:
                if c > self.best_inliers:
                    self.best, self.best_inliers = h, c; self.best_ref += 1
                    assert self.rec[self.best_ref] == h
                if self.ref_counts[self.best_ref] > self.min_inliers:
                    return ("refined", self.best), False, self._vb(self.ref_masks[self.best_ref]), self.ref_counts[self.best_ref]
        if self.best_inliers >= self.min_inliers:
            return ("best", self.best), True, self._vb(self.masks[self.best]), self.best_inliers
        return None, True, empty, 0


# ------------------------------------------------------------------------------------------------------ problem generators
def _rotation(rng, angle):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx


def make_problem(rng, n, wrong=0.3, noise=0.5, holes=0.25):
    """One PnPsolver's constructor data: n correspondences of a frame with a known pose.  The points lie in front of the camera
    (depth 2 .. 10); a share `wrong` of the matches points at an unrelated pixel; the others carry Gaussian pixel noise.  All
    values are stored as float32; sigma2 = 1.2^(2 level).  n1 > n: a share `holes` of the frame's keypoints has no map point."""
    K = np.array([520.0 + rng.uniform(-20, 20), 520.0 + rng.uniform(-20, 20), 320.0 + rng.uniform(-8, 8), 240.0 + rng.uniform(-8, 8)])
    R = _rotation(rng, rng.uniform(0.1, 1.2)); t = rng.uniform(-2, 2, 3)
    z = rng.uniform(2, 10, n)
    uv = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)], 1)
    Xc = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], 1)
    Xw = ((Xc - t) @ R).astype("f4")                                # R^T (Xc - t)
    bad = rng.random(n) < wrong
    obs = uv + rng.normal(0, noise, (n, 2))
    obs[bad] = np.stack([rng.uniform(0, 640, int(bad.sum())), rng.uniform(0, 480, int(bad.sum()))], 1)
    level = rng.integers(0, 8, n)
    n1 = n + int(round(holes * n)) + 1
    kp_index = np.sort(rng.choice(n1, n, replace=False)).astype("i4")
    return dict(K=K.astype("f4"), P2D=obs.astype("f4"), P3Dw=Xw, sigma2=(1.2 ** (2 * level)).astype("f4"), kp_index=kp_index, n1=n1,
                R=R, t=t, bad=bad)


def flatten(problems):
    cat = lambda k, shape, dt: np.concatenate([p[k].reshape(shape) for p in problems]) if problems else np.zeros((0,) + shape[1:], dt)
    first = np.concatenate([[0], np.cumsum([len(p["P2D"]) for p in problems])]).astype("i4")
    return dict(first=first, n1=np.array([p["n1"] for p in problems], "i4"), K=np.array([p["K"] for p in problems], "f4").reshape(-1, 4),
                P2D=cat("P2D", (-1, 2), "f4"), P3Dw=cat("P3Dw", (-1, 3), "f4"), sigma2=cat("sigma2", (-1,), "f4"),
                kp_index=cat("kp_index", (-1,), "i4"))


# ---------------------------------------------------------------------------------------- the tolerance rule for a tapped pose
def pose_tolerance(rng, pw, us, K, cws, basis):
    """The restatement fed with (cws, basis), and its own sensitivity: the deviation d of (R, t relative) when the basis is
    perturbed by a relative 1e-11 (Gaussian).  -> (restatement, d); d = inf for a non-finite restatement."""
    r = epnp(pw, us, K, cws, basis)
    p = epnp(pw, us, K, cws, np.asarray(basis) * (1 + 1e-11 * rng.normal(size=np.shape(basis))))
    if not (np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all() and np.isfinite(p["R"]).all() and np.isfinite(p["t"]).all()):
        return r, math.inf
    d = max(np.abs(r["R"] - p["R"]).max(), np.abs(r["t"] - p["t"]).max() / max(1.0, np.abs(r["t"]).max()))
    return r, d


def pose_agrees(R, t, which, rep_error, r, d):
    """The library's (R, t) against the restatement r within max(1e-9, 100 d) on R and relative on t; or against another beta
    candidate of r whose rep_error is within a relative 1e-9 of the chosen one's (a tie the two sides may break differently)."""
    tol = max(1e-9, 100 * d)
    for c in range(3):
        tie = c + 1 == r["which"] or abs(r["rep_error"][c] - r["rep_error"][r["which"] - 1]) <= 1e-9 * abs(r["rep_error"][r["which"] - 1])
        if tie and np.abs(R - r["Rs"][c]).max() <= tol and np.abs(t - r["ts"][c]).max() <= tol * max(1.0, np.abs(r["ts"][c]).max()):
            return True
    return False
