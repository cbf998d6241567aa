"""Mirror of cslam::Initializer (src/Initializer.cpp, include/cslam/Initializer.h:52-120) over the C ABI.

The constructor fixes the reference frame (:29-37); Initialize (:40-117) is one ccm_initialize call: every homography and
fundamental-matrix hypothesis in one launch, CheckRT of all motion candidates in a second one, the ordered selection and the
decisions replayed on the host.  The random draws of the minimal sets stay with the caller (make_draws), as for the Sim3Solver.
hypotheses() / candidates() return what the last Initialize stored per set and per motion candidate.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def make_draws(rng, n_matches: int, max_iterations: int = 200) -> np.ndarray:
    """What DUtils::Random::RandomInt(0, vAvailableIndices.size()-1) returns at src/Initializer.cpp:85, from a numpy Generator:
    draws[it, j] uniform in [0, N - 1 - j] (all 0 for N < 8, where nothing is evaluated)."""
    if n_matches < 8:
        return np.zeros((int(max_iterations), 8), "i4")
    hi = int(n_matches) - np.arange(8)                                                   # exclusive bound N - j
    return rng.integers(0, np.broadcast_to(hi, (int(max_iterations), 8))).astype("i4")


class Initializer:
    def __init__(self, kp1_xy, K, sigma: float = 1.0, iterations: int = 200, ctx=None):
        """kp1_xy [n1][2]: mvKeysUn of the reference frame; K: fx, fy, cx, cy (or the 3x3 matrix)."""
        self.ctx = ctx or _lib.default_context(0)
        self.lib = self.ctx.lib
        self.kp1 = np.ascontiguousarray(kp1_xy, "f4").reshape(-1, 2)
        K = np.asarray(K, "f4")
        self.K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], "f4") if K.shape == (3, 3) else K.reshape(4).copy()
        self.sigma, self.iterations = float(sigma), int(iterations)
        self.min_parallax, self.min_triangulated = 1.0, 50                               # the arguments of :112 / :114
        self.result = None
        self._tap = None

    def Initialize(self, kp2_xy, matches12, draws):
        """-> (ok, R21 [3][3], t21 [3], vP3D [n1][3], vbTriangulated [n1] bool); R21 / t21 are None when ok is False."""
        kp2 = np.ascontiguousarray(kp2_xy, "f4").reshape(-1, 2)
        m12 = np.ascontiguousarray(matches12, "i4").reshape(-1)
        if len(m12) != len(self.kp1):
            raise ValueError("matches12 has %d entries, the reference frame %d keypoints" % (len(m12), len(self.kp1)))
        draws = np.ascontiguousarray(draws, "i4").reshape(-1, 8)
        if len(draws) < self.iterations:
            raise ValueError("draws holds %d sets, iterations is %d" % (len(draws), self.iterations))
        n1, its = len(self.kp1), self.iterations
        n = int((m12 >= 0).sum()); words = max((n + 63) // 64, 1)
        t = dict(H21=np.zeros((its, 3, 3), "f4"), H12=np.zeros((its, 3, 3), "f4"), F21=np.zeros((its, 3, 3), "f4"),
                 score_h=np.zeros(its, "f4"), score_f=np.zeros(its, "f4"), mask_h=np.zeros((its, words), "u8"),
                 mask_f=np.zeros((its, words), "u8"), sets=np.zeros((its, 8), "i4"), cand_flags=np.zeros((8, max(n, 1)), "u1"),
                 cand_cos=np.zeros((8, max(n, 1)), "f4"), cand_p3d=np.zeros((8, max(n, 1), 3), "f4"))
        p = _lib.ptr
        tap = _lib.InitializerTap(p(t["H21"]), p(t["H12"]), p(t["F21"]), p(t["score_h"]), p(t["score_f"]), p(t["mask_h"]), p(t["mask_f"]),
                                  p(t["sets"]))
        tap.cand_flags, tap.cand_cos, tap.cand_p3d = p(t["cand_flags"]), p(t["cand_cos"]), p(t["cand_p3d"])
        p3d = np.zeros((max(n1, 1), 3), "f4"); tri = np.zeros(max(n1, 1), "u1")
        pb = _lib.InitializerProblem(n1, p(self.kp1), len(kp2), p(kp2), p(m12), *[float(x) for x in self.K], self.sigma, its,
                                     self.min_parallax, self.min_triangulated, p(draws))
        res = _lib.InitializerResult()
        res.p3d, res.triangulated, res.tap = p(p3d), p(tri), C.pointer(tap)
        self.ctx.check(self.lib.ccm_initialize(self.ctx.handle, C.byref(pb), C.byref(res)))
        self.result = dict(initialized=bool(res.initialized), model=int(res.model), score_h=np.float32(res.score_h),
                           score_f=np.float32(res.score_f), best_h=int(res.best_h), best_f=int(res.best_f), n_matches=int(res.n_matches))
        self._tap = (t, tap, n)
        ok = bool(res.initialized)
        R21 = np.array(res.R21, "f4").reshape(3, 3) if ok else None
        t21 = np.array(res.t21, "f4") if ok else None
        return ok, R21, t21, p3d[:n1], tri[:n1].astype(bool)

    def hypotheses(self) -> dict:
        """Per set of the last Initialize: sets [it][8], H21 / H12 / F21 [it][3][3], score_h / score_f [it], inlier_h / inlier_f
        [it][N] bool (match i in mvMatches12 order)."""
        t, _, n = self._tap
        idx = np.arange(n)
        bits = lambda m: ((m[:, idx // 64] >> (idx % 64).astype("u8")) & np.uint64(1)).astype(bool)
        if n < 8:
            return dict(sets=t["sets"][:0], H21=t["H21"][:0], H12=t["H12"][:0], F21=t["F21"][:0], score_h=t["score_h"][:0],
                        score_f=t["score_f"][:0], inlier_h=np.zeros((0, n), bool), inlier_f=np.zeros((0, n), bool))
        return dict(sets=t["sets"], H21=t["H21"], H12=t["H12"], F21=t["F21"], score_h=t["score_h"], score_f=t["score_f"],
                    inlier_h=bits(t["mask_h"]), inlier_f=bits(t["mask_f"]))

    def candidates(self) -> dict:
        """Per motion candidate of the last Initialize (8 for ReconstructH, 4 for ReconstructF, 0 if none was tested): R [k][3][3],
        t [k][3], n_good [k], parallax [k], and per match good / triangulated [k][N] bool, cos [k][N], p3d [k][N][3]."""
        t, tap, n = self._tap
        k = int(tap.n_candidates)
        return dict(R=np.array(tap.cand_R, "f4").reshape(8, 3, 3)[:k], t=np.array(tap.cand_t, "f4").reshape(8, 3)[:k],
                    n_good=np.array(tap.cand_n_good, "i4")[:k], parallax=np.array(tap.cand_parallax, "f4")[:k],
                    good=(t["cand_flags"][:k, :n] & 1).astype(bool), triangulated=(t["cand_flags"][:k, :n] >> 1 & 1).astype(bool),
                    cos=t["cand_cos"][:k, :n], p3d=t["cand_p3d"][:k, :n])
