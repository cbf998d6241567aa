"""Batched mirror of cslam::PnPsolver (src/PnPSolver.cpp, include/cslam/PnPSolver.h) over the C ABI.

One object holds the solvers of all relocalisation candidates of a frame.  Every minimal-set hypothesis of every solver is evaluated
in one launch and every reachable Refine() in a second one (ccm_pnp_solver_create); iterate / find replay the reference's ordered
bookkeeping over the stored results, so 5 iterations at a time round-robin (ORB-SLAM's Tracking::Relocalization), find(), or a
candidate resumed after its pose failed the optimisation return what the sequential code returns for the same random draws.

The RANSAC parameters are part of the create call, so the batch is evaluated lazily: at the first iterate / find after the last
SetRansacParameters.  Unlike the reference (:111-147), SetRansacParameters starts again from mnBestInliers = 0.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

DETAIL = 68     # CCM_PNP_DETAIL
PNP_HPB, PNP_TILE = 16, 1024    # csrc/pnp_types.h: hypotheses per workgroup, correspondences per LDS tile (the sizes tests straddle)


def make_draws(rng, n_correspondences, rows: int, min_set: int = 4) -> np.ndarray:
    """What DUtils::Random::RandomInt(0, vAvailableIndices.size()-1) returns at src/PnPSolver.cpp:183, from a numpy Generator:
    draws[k, h, i] uniform in [0, N_k - 1 - i] (0 where a solver has too few correspondences; it evaluates nothing)."""
    n = np.asarray(n_correspondences, "i8").reshape(-1)
    hi = np.maximum(n[:, None, None] - np.arange(min_set)[None, None, :], 1)          # exclusive bound N - i
    return rng.integers(0, np.broadcast_to(hi, (len(n), int(rows), min_set))).astype("i4")


def split_detail(d: np.ndarray) -> dict:
    """One or more rows of the detail tap -> cws [..][4][3], basis [..][4][12], betas [..][4], rep_error [..][3], which [..]."""
    d = np.asarray(d, "f8")
    lead = d.shape[:-1]
    return dict(cws=d[..., :12].reshape(lead + (4, 3)), basis=d[..., 12:60].reshape(lead + (4, 12)), betas=d[..., 60:64],
                rep_error=d[..., 64:67], which=d[..., 67].astype("i4"))


def ransac_parameters(n, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4):
    """SetRansacParameters (:119-142) for N = n: (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon).  Host only."""
    mi, it, eps = C.c_int32(), C.c_int32(), C.c_float()
    rc = _lib.load().ccm_pnp_ransac_parameters(int(n), float(probability), int(minInliers), int(maxIterations), int(minSet), float(epsilon),
                                               C.byref(mi), C.byref(it), C.byref(eps))
    if rc < 0:
        raise _lib.CcmError(rc, "ccm_pnp_ransac_parameters")
    return mi.value, it.value, eps.value


def compute_pose(P3Dw, P2D, K, detail: bool = False):
    """EPnP compute_pose (:468-516) on the host, the arithmetic of the kernels: (R [3][3], t [3]) float64, and the detail dict."""
    a = np.ascontiguousarray
    P3 = a(P3Dw, "f4").reshape(-1, 3); P2 = a(P2D, "f4").reshape(-1, 2); Kf = a(K, "f4").reshape(4)
    Rt = np.zeros(12, "f8"); d = np.zeros(DETAIL, "f8")
    rc = _lib.load().ccm_pnp_compute_pose(len(P3), _lib.ptr(P3), _lib.ptr(P2), _lib.ptr(Kf), _lib.ptr(Rt), _lib.ptr(d) if detail else None)
    if rc < 0:
        raise _lib.CcmError(rc, "ccm_pnp_compute_pose")
    R, t = Rt[:9].reshape(3, 3), Rt[9:]
    return (R, t, split_detail(d)) if detail else (R, t)


class PnPSolver:
    def __init__(self, first, n1, K, P2D, P3Dw, sigma2, kp_index, draws, reserve: int = 0, detail: bool = False, ctx=None):
        """The constructor data of n solvers (:57-100), flattened: correspondences of solver k are rows first[k] .. first[k+1]-1 of
        P2D (mvKeysUn[i].pt), P3Dw (GetWorldPos), sigma2 (mvLevelSigma2[octave]) and kp_index (mvKeyPointIndices); n1[k] =
        mvpMapPointMatches.size(); K [n][4] = fx, fy, cx, cy.  draws [n][>= maxIterations + reserve][minSet]: see make_draws.
        reserve: hypotheses kept past mRansacMaxIts for iterate's || (the caller's nIterations covers every caller that drops a
        solver at bNoMore)."""
        a = np.ascontiguousarray
        self.ctx = ctx or _lib.default_context(0)
        self.lib = _lib.load()
        self.first = a(first, "i4"); self.n = len(self.first) - 1
        self.n1 = a(n1, "i4").reshape(-1)
        self.K = a(K, "f4").reshape(-1, 4)
        self.P2D = a(P2D, "f4").reshape(-1, 2); self.P3Dw = a(P3Dw, "f4").reshape(-1, 3)
        self.sigma2 = a(sigma2, "f4").reshape(-1); self.kp_index = a(kp_index, "i4").reshape(-1)
        self.draws = np.asarray(draws, "i4")
        self.reserve, self.detail = int(reserve), bool(detail)
        self._handle = None
        self.SetRansacParameters()                      # :99

    @classmethod
    def from_frames(cls, cur, table, first, K, feature, slot, level_sigma2, draws, reserve: int = 0, detail: bool = False, ctx=None):
        """The same solvers with the constructor's loop on the device (ccm_pnp_solver_create_frames): correspondence e is feature
        feature[e] of the DeviceFrame `cur` and slot[e] of the MapPointTable `table` -- the features i whose vpMapPointMatches[i] is
        set and not bad, in i order, and that point's slot.  P2D, P3Dw, sigma2 and kp_index are not passed: the keypoints and
        octaves come from the handle, the positions from the table; n1 is the frame's feature count for every solver."""
        a = np.ascontiguousarray
        self = cls.__new__(cls)
        self.ctx = ctx or cur.ctx
        self.lib = _lib.load()
        self.first = a(first, "i4"); self.n = len(self.first) - 1
        self.n1 = np.full(max(self.n, 1), cur.n, "i4")[:self.n]
        self.K = a(K, "f4").reshape(-1, 4)
        self.kp_index = a(feature, "i4").reshape(-1); self.slot = a(slot, "i4").reshape(-1)
        if len(self.kp_index) != len(self.slot):
            raise ValueError("feature and slot differ in length")
        self.level_sigma2 = a(level_sigma2, "f4").reshape(-1)
        self.frames = (cur, table)
        self.draws = np.asarray(draws, "i4")
        self.reserve, self.detail = int(reserve), bool(detail)
        self._handle = None
        self.SetRansacParameters()
        return self

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 8, maxIterations: int = 300, minSet: int = 4,
                            epsilon: float = 0.4, th2: float = 5.991):
        self.close()
        self.probability, self.min_inliers, self.max_iterations = float(probability), int(minInliers), int(maxIterations)
        self.min_set, self.epsilon, self.th2 = int(minSet), float(epsilon), float(th2)

    def _ensure(self):
        if self._handle is not None:
            return
        rows = self.max_iterations + self.reserve
        d = self.draws.reshape(self.n, -1, self.min_set) if self.n else np.zeros((0, rows, self.min_set), "i4")
        if self.n and d.shape[1] < rows:
            raise ValueError("draws holds %d hypotheses per solver, maxIterations + reserve is %d" % (d.shape[1], rows))
        d = np.ascontiguousarray(d[:, :rows])
        p = _lib.ptr
        h = C.c_void_p()
        if getattr(self, "frames", None) is not None:
            cur, table = self.frames
            fp = _lib.PnpFramesProblem(self.n, p(self.first), p(self.K), p(self.kp_index), p(self.slot), p(self.level_sigma2),
                                       len(self.level_sigma2), self.probability, self.min_inliers, self.max_iterations, self.min_set,
                                       self.epsilon, self.th2, self.reserve, p(d), 1 if self.detail else 0)
            self.ctx.check(self.lib.ccm_pnp_solver_create_frames(self.ctx.handle, C.c_void_p(cur.handle), C.c_void_p(table.handle), C.byref(fp), C.byref(h)))
            self._handle = h
            return
        pb = _lib.PnpRansacProblem(self.n, p(self.first), p(self.n1), p(self.K), p(self.P2D), p(self.P3Dw), p(self.sigma2), p(self.kp_index),
                                   self.probability, self.min_inliers, self.max_iterations, self.min_set, self.epsilon, self.th2,
                                   self.reserve, p(d), 1 if self.detail else 0)
        self.ctx.check(self.lib.ccm_pnp_solver_create(self.ctx.handle, C.byref(pb), C.byref(h)))
        self._handle = h

    def _check(self, rc):
        if rc < 0:
            raise _lib.CcmError(rc, "PnPSolver")
        return rc

    def iterate(self, k: int, nIterations: int):
        """PnPsolver::iterate of solver k (:155-249): (Tcw 4x4 float32 or None, bNoMore, vbInliers [n1] bool, nInliers)."""
        self._ensure()
        found, no_more, nin = C.c_int32(), C.c_int32(), C.c_int32()
        inl = np.zeros(max(int(self.n1[k]), 1), np.uint8); T = np.zeros((4, 4), "f4")
        self._check(self.lib.ccm_pnp_solver_iterate(self._handle, int(k), int(nIterations), C.byref(found), C.byref(no_more), _lib.ptr(inl),
                                                    C.byref(nin), _lib.ptr(T)))
        return (T if found.value else None), bool(no_more.value), inl[:self.n1[k]].astype(bool), nin.value

    def find(self, k: int):
        """PnPsolver::find (:149-153): (Tcw or None, vbInliers, nInliers)."""
        self._ensure()
        found, nin = C.c_int32(), C.c_int32()
        inl = np.zeros(max(int(self.n1[k]), 1), np.uint8); T = np.zeros((4, 4), "f4")
        self._check(self.lib.ccm_pnp_solver_find(self._handle, int(k), C.byref(found), _lib.ptr(inl), C.byref(nin), _lib.ptr(T)))
        return (T if found.value else None), inl[:self.n1[k]].astype(bool), nin.value

    def state(self, k: int) -> dict:
        """mnIterations, mnBestInliers, the hypothesis behind the running best (-1: none), mRansacMaxIts, mRansacMinInliers."""
        self._ensure()
        v = [C.c_int32() for _ in range(5)]
        self._check(self.lib.ccm_pnp_solver_state(self._handle, int(k), *[C.byref(x) for x in v]))
        return dict(iterations=v[0].value, best_inliers=v[1].value, best_hypothesis=v[2].value, max_iterations=v[3].value,
                    min_inliers=v[4].value)

    def _tap(self, fn, k, width):
        n = int(self.first[k + 1] - self.first[k]); words = (n + 63) // 64
        H = self._check(fn(self._handle, int(k), None, None, None, None, None))
        first = np.zeros((H, width), "i4"); count = np.zeros(H, "i4"); Rt = np.zeros((H, 12), "f8"); mask = np.zeros((H, max(words, 1)), "u8")
        det = np.zeros((H, DETAIL), "f8")
        if H:
            self._check(fn(self._handle, int(k), _lib.ptr(first), _lib.ptr(count), _lib.ptr(Rt), _lib.ptr(mask), _lib.ptr(det) if self.detail else None))
        bits = (mask[:, np.arange(n) // 64] >> (np.arange(n) % 64).astype("u8")) & np.uint64(1) if n else np.zeros((H, 0), "u8")
        out = dict(count=count, Rt=Rt, R=Rt[:, :9].reshape(H, 3, 3), t=Rt[:, 9:], inlier=bits.astype(bool))
        if self.detail:
            out.update(split_detail(det))
        return first, out

    def hypotheses(self, k: int) -> dict:
        """What the first launch stored for solver k: sample [H][minSet], count [H], Rt [H][12] / R / t float64, inlier [H][N] bool,
        and with detail=True cws, basis, betas, rep_error, which."""
        self._ensure()
        first, out = self._tap(self.lib.ccm_pnp_solver_hypotheses, k, self.min_set)
        out["sample"] = first
        return out

    def refinements(self, k: int) -> dict:
        """One row per record hypothesis (a hypothesis that becomes the running best), in order: hyp [R], count, Rt, inlier, ..."""
        self._ensure()
        first, out = self._tap(self.lib.ccm_pnp_solver_refinements, k, 1)
        out["hyp"] = first[:, 0]
        return out

    compute_pose = staticmethod(compute_pose)
    ransac_parameters = staticmethod(ransac_parameters)

    def close(self):
        if getattr(self, "_handle", None) is not None:
            self.lib.ccm_pnp_solver_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
