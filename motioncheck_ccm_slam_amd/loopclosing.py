"""LoopFinder::ComputeSim3 / MapMatcher::ComputeSim3 from the RANSAC round-robin on (src/LoopFinder.cpp:284-346,
src/MapMatcher.cpp:288-350), on keyframe handles and the map-point table.

The reference runs, per candidate and per pass, iterate(5) and -- where a Sim3 comes back -- SearchBySim3 and OptimizeSim3, and
stops at the first candidate whose optimisation keeps mInliersThres inliers.  Here a pass first iterates every live candidate, in
order, on the solvers' host replay (sim3solver.Sim3Solver), and then makes ONE chain call (ccm_compute_sim3_table_frames) for the
candidates that returned a Sim3."""
from __future__ import annotations

import numpy as np


def sim3_matrices(R, t, s):
    """The two [3][4] float matrices ORBmatcher::SearchBySim3 forms of R12, t12, s12 (src/ORBmatcher.cpp:1141-1143): rows of
    [s R12 | t12] and of [(1 / s) R12^T | -sR21 t12], float storage, the matrix product summed in double."""
    R = np.ascontiguousarray(R, "f4").reshape(3, 3); t = np.ascontiguousarray(t, "f4").reshape(3); s = np.float32(s)
    sR12 = (s * R).astype("f4")
    sR21 = ((1.0 / np.float64(s)) * R.T.astype("f8")).astype("f4")
    t21 = (-(sR21.astype("f8") @ t.astype("f8"))).astype("f4")
    return np.concatenate([sR12, t[:, None]], 1).astype("f4"), np.concatenate([sR21, t21[:, None]], 1).astype("f4")


def g2o_sim3(R, t, s):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s) as qx, qy, qz, qw, tx, ty, tz, s: the floats widened, the
    quaternion by Eigen's conversion from a rotation matrix (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl)."""
    m = np.ascontiguousarray(R, "f4").reshape(3, 3).astype("f8")
    q = np.zeros(4)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        r = np.sqrt(tr + 1.0)
        q[3] = 0.5 * r
        r = 0.5 / r
        q[0] = (m[2, 1] - m[1, 2]) * r; q[1] = (m[0, 2] - m[2, 0]) * r; q[2] = (m[1, 0] - m[0, 1]) * r
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        r = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * r
        r = 0.5 / r
        q[3] = (m[k, j] - m[j, k]) * r; q[j] = (m[j, i] + m[i, j]) * r; q[k] = (m[k, i] + m[i, k]) * r
    return np.concatenate([q, np.ascontiguousarray(t, "f4").reshape(3).astype("f8"), [np.float64(np.float32(s))]])


def ComputeSim3(solver, chain, discarded=None, mInliersThres: int = 20, mSolverIterations: int = 5):
    """The loop of src/LoopFinder.cpp:284-346.  solver: a sim3solver.Sim3Solver (or anything with n, iterate(k, nIterations) ->
    (T12 or None, bNoMore, vbInliers, nInliers) and GetEstimatedRotation / Translation / Scale(k)).  chain(items) -> one dict per item
    with at least n_inliers, for items = [(candidate, vbInliers, R, t, s), ...]: SearchBySim3 and OptimizeSim3 for those candidates,
    e.g. SearchAndOptimize below.  discarded: vbDiscarded on entry.  Returns None when every candidate is used up, else the chain's
    dict of the matched candidate with `candidate` and `inliers` (vbInliers of that iterate) added.

    Per pass every live candidate is iterated in order, then one chain call is made for those that returned a Sim3, and the first
    of them, in candidate order, with n_inliers >= mInliersThres wins.  That is what the sequential loop returns: the candidates
    behind the winner have advanced their solver by one iterate() the sequential loop would not have made, which nothing can
    observe after a match (the solvers are dropped), and when no candidate of a pass matches both orders have made the same calls."""
    n = solver.n
    vbDiscarded = [False] * n if discarded is None else [bool(x) for x in discarded]
    nCandidates = n - sum(vbDiscarded)
    while nCandidates > 0:
        items = []
        for i in range(n):
            if vbDiscarded[i]:
                continue
            Scm, bNoMore, vbInliers, _ = solver.iterate(i, mSolverIterations)
            if bNoMore:
                vbDiscarded[i] = True
                nCandidates -= 1
            if Scm is not None:
                items.append((i, vbInliers, solver.GetEstimatedRotation(i), solver.GetEstimatedTranslation(i), solver.GetEstimatedScale(i)))
        if not items:
            continue
        for item, res in zip(items, chain(items)):
            if res["n_inliers"] >= mInliersThres:
                return dict(res, candidate=item[0], inliers=item[1])
    return None


class SearchAndOptimize:
    """chain for ComputeSim3 over ORBmatcher.ComputeSim3TableFrames: candidate k is pairs[k] -- a dict of that call without matched12,
    matched_idx2, S12, S21 and sim3, which come from the solver -- with bow12[k] / bow_idx2[k] [N1]: vvpMapPointMatches[k] as table
    slots (or -1) and the features of the candidate that hold them.  A result carries, besides the call's own entries of the pair,
    matches [N1]: vpMapPointMatches after OptimizeSim3 as features of the candidate keyframe, or -1."""

    def __init__(self, matcher, table, pairs, bow12, bow_idx2, scale_factors, inv_level_sigma2, th: float = 7.5, log_scale_factor=None):
        self.matcher, self.table, self.pairs = matcher, table, pairs
        self.bow12 = [np.asarray(x, "i4") for x in bow12]; self.bow_idx2 = [np.asarray(x, "i4") for x in bow_idx2]
        self.sf, self.is2, self.th, self.log_sf = scale_factors, inv_level_sigma2, th, log_scale_factor

    def pair(self, item):
        k, inl, R, t, s = item
        S12, S21 = sim3_matrices(R, t, s)
        keep = np.asarray(inl, bool)
        return dict(self.pairs[k], matched12=np.where(keep, self.bow12[k], -1).astype("i4"), matched_idx2=np.where(keep, self.bow_idx2[k], -1).astype("i4"),
                    S12=S12, S21=S21, sim3=g2o_sim3(R, t, s))

    def __call__(self, items):
        pairs = [self.pair(it) for it in items]
        r = self.matcher.ComputeSim3TableFrames(self.table, pairs, self.sf, self.is2, th=self.th, log_scale_factor1=self.log_sf)
        out = []
        for j, p in enumerate(pairs):
            m = np.where(p["matched12"] >= 0, p["matched_idx2"], r["match12"][j])
            m = np.where(r["pruned"][j] != 0, -1, m).astype("i4")
            out.append(dict(n_inliers=r["n_inliers"][j], sim3=r["sim3"][j].copy(), matches=m, match12=r["match12"][j], pruned=r["pruned"][j],
                            n_correspondences=r["n_correspondences"][j], n_found=r["n_found"][j]))
        return out
