"""Batched mirror of cslam::Sim3Solver (src/Sim3Solver.cpp, include/cslam/Sim3Solver.h:28-124) over the C ABI.

One object holds the solvers of all candidate keyframes of a loop / map-match query.  Every hypothesis of every solver is
evaluated in one launch (ccm_sim3_solver_create); iterate / find replay the reference's ordered bookkeeping over the stored
results, so 5 iterations at a time round-robin (src/LoopFinder.cpp:284-346), find(), or a candidate resumed after its estimate
failed OptimizeSim3 return what the sequential code returns for the same random draws.

The RANSAC parameters are part of the create call, so the batch is evaluated lazily: at the first iterate / find after the last
SetRansacParameters.  As in the reference (:94-118) SetRansacParameters resets mnIterations but not mnBestInliers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def make_draws(rng, n_correspondences, max_iterations: int) -> np.ndarray:
    """What DUtils::Random::RandomInt(0, vAvailableIndices.size()-1) returns at src/Sim3Solver.cpp:151, from a numpy Generator:
    draws[k, h, i] uniform in [0, N_k - 1 - i] (0 where a solver has fewer than 3 correspondences; it evaluates nothing)."""
    n = np.asarray(n_correspondences, "i8").reshape(-1)
    hi = np.maximum(n[:, None, None] - np.arange(3)[None, None, :], 1)                 # exclusive bound N - i
    return rng.integers(0, np.broadcast_to(hi, (len(n), int(max_iterations), 3))).astype("i4")


def level_max_err(level_sigma2) -> np.ndarray:
    """mvnMaxError per pyramid level: 9.210 * mvLevelSigma2[level] (src/Sim3Solver.cpp:67) pushed into a std::vector<size_t>
    (include/cslam/Sim3Solver.h:74-75), which drops the fraction, and read back as a float."""
    return np.trunc(9.210 * np.asarray(level_sigma2, "f4").astype("f8")).astype("f4")


def fill_frames_pair(rec, q):
    """A ccm_sim3_frames_pair from a dict kf1, kf2, T1w, T2w, K1, K2."""
    rec.kf1 = q["kf1"].handle; rec.kf2 = q["kf2"].handle
    for name, n in (("T1w", 12), ("T2w", 12), ("K1", 4), ("K2", 4)):
        getattr(rec, name)[:] = [float(x) for x in np.ascontiguousarray(q[name], "f4").reshape(n)]


class Sim3Solver:
    def __init__(self, first, n1, X1, X2, max_err1, max_err2, indices1, K1, K2, fix_scale, draws, ctx=None):
        """The constructor data of n solvers (:5-92), flattened: correspondences of solver k are rows first[k] .. first[k+1]-1 of
        X1 / X2 (mvX3Dc1 / mvX3Dc2, float32 camera-frame points), max_err1 / max_err2 (9.210 * mvLevelSigma2[octave]) and
        indices1 (mvnIndices1); n1[k] = mN1; K1 / K2 [n][4] = fx, fy, cx, cy; fix_scale per solver or one flag.
        draws [n][>= maxIterations][3]: see make_draws."""
        a = np.ascontiguousarray
        self.ctx = ctx or _lib.default_context(0)
        self.lib = _lib.load()
        self.first = a(first, "i4"); self.n = len(self.first) - 1
        self.n1 = a(n1, "i4").reshape(-1)
        self.X1 = a(X1, "f4").reshape(-1, 3); self.X2 = a(X2, "f4").reshape(-1, 3)
        self.max_err1 = a(max_err1, "f4").reshape(-1); self.max_err2 = a(max_err2, "f4").reshape(-1)
        self.indices1 = a(indices1, "i4").reshape(-1)
        self.K1 = a(K1, "f4").reshape(-1, 4); self.K2 = a(K2, "f4").reshape(-1, 4)
        self.fix_scale = a(np.broadcast_to(np.asarray(fix_scale, "i4"), (self.n,)), "i4")
        self.draws = np.asarray(draws, "i4").reshape(self.n, -1, 3) if self.n else np.zeros((0, 0, 3), "i4")
        self._handle = None
        self._best0 = np.zeros(self.n, "i4")            # mnBestInliers carried over a SetRansacParameters
        self._prev = [None] * self.n                    # and the estimate that belongs to it
        self.SetRansacParameters()                      # :91

    @classmethod
    def from_frames(cls, table, pairs, first, feature1, feature2, max_err_level1, max_err_level2=None, fix_scale=False, draws=None, ctx=None):
        """The same solvers with the constructor's loop on the device (ccm_sim3_solver_create_frames): correspondence e of solver k
        is (feature1[e] of pairs[k]['kf1'], feature2[e] of pairs[k]['kf2']), its two map points the slots the handles hold there in
        `table`.  pairs: dicts kf1, kf2 (DeviceFrame handles), T1w, T2w ([12] or [3][4]), K1, K2 (fx, fy, cx, cy).  max_err_level:
        per pyramid level, (float)(size_t)(9.210 * mvLevelSigma2[level]) -- level_max_err() -- for either side."""
        a = np.ascontiguousarray
        self = cls.__new__(cls)
        self.ctx = ctx or _lib.default_context(0)
        self.lib = _lib.load()
        self.first = a(first, "i4"); self.n = len(self.first) - 1
        self.table = table; self.pairs = list(pairs)
        if len(self.pairs) != self.n:
            raise ValueError("one pair per solver")
        self.n1 = a([p["kf1"].n for p in self.pairs], "i4").reshape(-1)
        self.feature1 = a(feature1, "i4").reshape(-1); self.feature2 = a(feature2, "i4").reshape(-1)
        self.indices1 = self.feature1
        self.max_err_level1 = a(max_err_level1, "f4").reshape(-1)
        self.max_err_level2 = self.max_err_level1 if max_err_level2 is None else a(max_err_level2, "f4").reshape(-1)
        self.fix_scale = a(np.broadcast_to(np.asarray(fix_scale, "i4"), (self.n,)), "i4")
        self.draws = np.asarray(draws, "i4").reshape(self.n, -1, 3) if self.n else np.zeros((0, 0, 3), "i4")
        self._handle = None
        self._best0 = np.zeros(self.n, "i4"); self._prev = [None] * self.n
        self.SetRansacParameters()
        return self

    def frames_problem(self, draws, n_levels1=None, n_levels2=None):
        """The ccm_sim3_solver_frames_problem of this batch and the objects that keep its arrays alive."""
        recs = (_lib.Sim3FramesPair * max(self.n, 1))()
        for k, q in enumerate(self.pairs):
            fill_frames_pair(recs[k], q)
        p = _lib.ptr
        draws = np.ascontiguousarray(draws, "i4")
        pb = _lib.Sim3SolverFramesProblem(self.n, recs, p(self.first), p(self.fix_scale), p(self.feature1), p(self.feature2),
                                          len(self.max_err_level1) if n_levels1 is None else n_levels1, p(self.max_err_level1),
                                          len(self.max_err_level2) if n_levels2 is None else n_levels2, p(self.max_err_level2),
                                          self.probability, self.min_inliers, self.max_iterations, p(draws), p(self._best0))
        return pb, (recs, draws)

    def _create_frames(self, draws):
        pb, keep = self.frames_problem(draws)
        h = C.c_void_p()
        self.ctx.check(self.lib.ccm_sim3_solver_create_frames(self.ctx.handle, C.c_void_p(self.table.handle), C.byref(pb), C.byref(h)))
        self._handle = h

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 6, maxIterations: int = 300):
        if self._handle is not None:
            for k in range(self.n):
                self._best0[k] = self.state(k)["best_inliers"]
                est = self._estimate(k)
                if est is not None:
                    self._prev[k] = est
            self.close()
        self.probability, self.min_inliers, self.max_iterations = float(probability), int(minInliers), int(maxIterations)

    def _ensure(self):
        if self._handle is not None:
            return
        if self.n and self.draws.shape[1] < self.max_iterations:
            raise ValueError("draws holds %d hypotheses per solver, maxIterations is %d" % (self.draws.shape[1], self.max_iterations))
        draws = np.ascontiguousarray(self.draws[:, :self.max_iterations])
        if getattr(self, "table", None) is not None:
            return self._create_frames(draws)
        p = _lib.ptr
        pb = _lib.Sim3RansacProblem(self.n, p(self.first), p(self.n1), p(self.fix_scale), p(self.K1), p(self.K2), p(self.X1), p(self.X2),
                                    p(self.max_err1), p(self.max_err2), p(self.indices1), self.probability, self.min_inliers,
                                    self.max_iterations, p(draws), p(self._best0))
        h = C.c_void_p()
        self.ctx.check(self.lib.ccm_sim3_solver_create(self.ctx.handle, C.byref(pb), C.byref(h)))
        self._handle = h

    def _check(self, rc):
        if rc < 0:
            raise _lib.CcmError(rc, "Sim3Solver")
        return rc

    def iterate(self, k: int, nIterations: int):
        """Sim3Solver::iterate of solver k (:120-191): (T12 4x4 float32 or None, bNoMore, vbInliers [mN1] bool, nInliers)."""
        self._ensure()
        found, no_more, nin = C.c_int32(), C.c_int32(), C.c_int32()
        inl = np.zeros(max(int(self.n1[k]), 1), np.uint8); T = np.zeros((4, 4), "f4")
        self._check(self.lib.ccm_sim3_solver_iterate(self._handle, int(k), int(nIterations), C.byref(found), C.byref(no_more),
                                                     _lib.ptr(inl), C.byref(nin), _lib.ptr(T)))
        return (T if found.value else None), bool(no_more.value), inl[:self.n1[k]].astype(bool), nin.value

    def find(self, k: int):
        """Sim3Solver::find (:193-197): (T12 or None, vbInliers12, nInliers)."""
        self._ensure()
        found, nin = C.c_int32(), C.c_int32()
        inl = np.zeros(max(int(self.n1[k]), 1), np.uint8); T = np.zeros((4, 4), "f4")
        self._check(self.lib.ccm_sim3_solver_find(self._handle, int(k), C.byref(found), _lib.ptr(inl), C.byref(nin), _lib.ptr(T)))
        return (T if found.value else None), inl[:self.n1[k]].astype(bool), nin.value

    def _estimate(self, k):
        R = np.zeros((3, 3), "f4"); t = np.zeros(3, "f4"); s = C.c_float()
        rc = self.lib.ccm_sim3_solver_estimate(self._handle, int(k), _lib.ptr(R), _lib.ptr(t), C.byref(s))
        if rc == -7:                                    # CCM_E_STATE: no hypothesis has become the best yet
            return None
        self._check(rc)
        return R, t, s.value

    def _best(self, k):
        self._ensure()
        return self._estimate(k) or self._prev[k] or (None, None, None)

    def GetEstimatedRotation(self, k: int):
        return self._best(k)[0]

    def GetEstimatedTranslation(self, k: int):
        return self._best(k)[1]

    def GetEstimatedScale(self, k: int):
        return self._best(k)[2]

    def state(self, k: int) -> dict:
        """mnIterations, mnBestInliers, the hypothesis behind the running best (-1: none) and mRansacMaxIts of solver k."""
        self._ensure()
        v = [C.c_int32() for _ in range(4)]
        self._check(self.lib.ccm_sim3_solver_state(self._handle, int(k), *[C.byref(x) for x in v]))
        return dict(iterations=v[0].value, best_inliers=v[1].value, best_hypothesis=v[2].value, max_iterations=v[3].value)

    def hypotheses(self, k: int) -> dict:
        """What the launch stored for solver k: sample [H][3], count [H], R [H][3][3], t [H][3], s [H], inlier [H][N] bool."""
        self._ensure()
        n = int(self.first[k + 1] - self.first[k]); words = (n + 63) // 64
        H = self._check(self.lib.ccm_sim3_solver_hypotheses(self._handle, int(k), None, None, None, None))
        sample = np.zeros((H, 3), "i4"); count = np.zeros(H, "i4"); rts = np.zeros((H, 13), "f4"); mask = np.zeros((H, max(words, 1)), "u8")
        if H:
            self._check(self.lib.ccm_sim3_solver_hypotheses(self._handle, int(k), _lib.ptr(sample), _lib.ptr(count), _lib.ptr(rts), _lib.ptr(mask)))
        bits = (mask[:, np.arange(n) // 64] >> (np.arange(n) % 64).astype("u8")) & np.uint64(1) if n else np.zeros((H, 0), "u8")
        return dict(sample=sample, count=count, R=rts[:, :9].reshape(H, 3, 3), t=rts[:, 9:12], s=rts[:, 12], inlier=bits.astype(bool))

    def close(self):
        if getattr(self, "_handle", None) is not None:
            self.lib.ccm_sim3_solver_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
