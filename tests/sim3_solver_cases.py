"""Inputs of the Sim3Solver edge tests (tests/test_sim3_solver_cases_cpu.py, tests/test_sim3_solver_cases_gpu.py) and of the special-input
study in tools/sim3_ransac_study.py.  Everything here is numpy on the CPU; the solver problems are those of sim3_solver_ref.

  size_batch        N on the mask-word edges (63 .. 129), on the edges of the kernel's 1024-correspondence tile (1023 .. 1025) and
                    past two tiles (2049), at a MaxIterations of one workgroup's 64 hypotheses plus one
  exhaustive_batch  N = 3 .. 7 with every legal draw triple as the first rows
  degenerate / identity / half_turn   N = 70 (two mask words): coincident and collinear samples, z = 0, a point behind the camera,
                    bounds of 0, +inf and NaN; X1 = X2; X1 = diag(-1, -1, 1) X2 + t0
"""
import itertools

import numpy as np

import sim3_solver_ref as ref
from sim3_problems import sim3_map

PROB, MIN_INLIERS = 0.99, 6
SIZES = [63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049]
FIXED_SCALE = (65, 128, 1025)                          # the solvers of the size batch that keep s = 1
SEED = 41
TILE, HPB = 1024, 64                                   # S3R_TILE, S3R_HPB (csrc/sim3_ransac_types.h)
PLANTED = 8                                            # rows 0-5: the corner draws of :146-161; rows 6-7 (N > TILE): correct matches only


def make_draws(rng, sizes, max_iterations):
    """draws[k, h, i] uniform in [0, N_k - 1 - i]: what sim3solver.make_draws returns, restated so that this module needs no library"""
    n = np.asarray(sizes, "i8").reshape(-1)
    hi = np.maximum(n[:, None, None] - np.arange(3)[None, None, :], 1)
    return rng.integers(0, np.broadcast_to(hi, (len(n), int(max_iterations), 3))).astype("i4")


def corner_draws(n):
    """the corners of :146-161 the older GPU test plants: the last element, repeated values, position 0"""
    return np.array([[n - 1, n - 2, n - 3], [0, 0, 0], [n - 2, n - 2, 0], [1, 1, 1], [n - 1, 0, n - 3], [2, n - 2, 2]], "i4")


def correct_draws(p):
    """Two draws whose three correspondences are all correct matches, far apart, and together touch every tile: the first holds the
    last correspondence (a tile of its own at N = 1025 and 2049), the second one of each remaining tile or of the first."""
    n = len(p["X1"]); good = np.flatnonzero(~p["bad"])
    assert not p["bad"][n - 1], "the seed must leave the last correspondence a correct match"
    low = good[good < n - 3]                            # below n - 3 a draw selects the index it names (no swapped-in element)
    a = [n - 1, int(low[len(low) // 3]), int(low[2 * len(low) // 3])]
    b = [int(low[1]), int(low[len(low) // 2]), int(low[-1])]
    for d in (a, b):
        assert ref.sample_indices(n, d) == d and not p["bad"][d].any()
    return np.array([a, b], "i4")


def size_batch(max_iterations=65, sizes=SIZES, seed=SEED):
    """-> (problems, draws [len(sizes)][max_iterations][3]).  The problems and the first rows of the draws do not depend on
    max_iterations or on which sizes are asked for: a solver of a smaller batch is the same solver."""
    rng = np.random.default_rng(seed)
    problems = [ref.make_solver_problem(rng, n, 0.3, n in FIXED_SCALE) for n in SIZES]
    draws = make_draws(rng, SIZES, 65)
    for k, n in enumerate(SIZES):
        draws[k, :6] = corner_draws(n)
        if n > TILE:
            draws[k, 6:8] = correct_draws(problems[k])
    keep = [SIZES.index(n) for n in sizes]
    return [problems[k] for k in keep], np.ascontiguousarray(draws[keep][:, :max_iterations])


def all_triples(n):
    """every legal draw triple of a solver with n correspondences: r_i in [0, n - 1 - i]"""
    return np.array(list(itertools.product(range(n), range(n - 1), range(n - 2))), "i4").reshape(-1, 3)


EXHAUSTIVE_SIZES = [3, 4, 5, 6, 7]
EXHAUSTIVE_MIN_INLIERS, EXHAUSTIVE_MAX_ITS = 1, 210


def exhaustive_batch(seed=43):
    """N = 3 .. 7, MinInliers 1, MaxIterations 210: SetRansacParameters gives 123, 210, 210, 210, 210 hypotheses, at least the
    N (N-1) (N-2) = 6, 24, 60, 120, 210 legal triples, which are the first rows; the rest is random."""
    rng = np.random.default_rng(seed)
    problems = [ref.make_solver_problem(rng, n, 0.0, False) for n in EXHAUSTIVE_SIZES]
    draws = make_draws(rng, EXHAUSTIVE_SIZES, EXHAUSTIVE_MAX_ITS)
    for k, n in enumerate(EXHAUSTIVE_SIZES):
        t = all_triples(n)
        assert len(t) == n * (n - 1) * (n - 2) <= ref.ransac_iterations(n, PROB, EXHAUSTIVE_MIN_INLIERS, EXHAUSTIVE_MAX_ITS)
        draws[k, :len(t)] = t
    return problems, draws


# ---------------------------------------------------------------- special inputs, N = 70
SPECIAL_N, SPECIAL_MAX_ITS = 70, 65
# float32 against float64 closed form on the identity and half-turn solvers below, as tools/sim3_ransac_study.py (study_special) prints
# it: max |dR|, max |dt| / max(1, |t|inf), max |ds| / s over the samples that span a triangle.  The GPU test's bounds are 4 x these.
SPECIAL_MEASURED = {"identity, free scale": (0.0, 4.77e-07, 5.96e-08), "identity, fixed scale": (0.0, 0.0, 0.0),
                    "half turn": (2.05e-06, 2.39e-06, 8.8e-08)}


def degenerate(seed=44):
    """A normal problem with, in this order of rows: 0-2 one point in frame 2 (den = 0: s = NaN), 3-5 one point in frame 1 (nom = 0:
    s = 0, 1 / s = inf), both with coordinates whose centroid is exact, 6-8 on one line in both frames (steps exact in float32), 9 with z = 0 in frame 1, 10 with z = 0 in frame 2, 11 behind camera 1, 12 with a bound of 0, 13 with a
    bound of +inf, 14 with a NaN bound.  Rows 9-14 start as exact images of their X2 under the true similarity, so that only the
    planted property keeps them from being inliers.  Draws 0-2 select rows (0,1,2), (3,4,5), (6,7,8)."""
    rng = np.random.default_rng(seed)
    p = ref.make_solver_problem(rng, SPECIAL_N, 0.3, False)
    X1, X2 = p["X1"].astype("f8"), p["X2"].astype("f8")
    X1[9:15] = sim3_map(p["S_true"], X2[9:15]); p["bad"][9:15] = False
    X2[0] = [-0.75, 0.5, 5.0]; X1[3] = [0.5, -0.75, 4.0]                     # (a + a + a) / 3 = a exactly: the centred sample is exactly 0
    X2[1] = X2[2] = X2[0]
    X1[4] = X1[5] = X1[3]
    X2[6] = [0.5, -0.25, 4.0]; X2[7] = X2[6] + [0.25, 0.125, 0.5]; X2[8] = X2[6] + [0.5, 0.25, 1.0]
    X1[6] = [0.75, 0.5, 3.0]; X1[7] = X1[6] + [-0.125, 0.25, 0.375]; X1[8] = X1[6] + [-0.25, 0.5, 0.75]
    X1[9, 2] = 0.0; X2[10, 2] = 0.0
    X1[11, 2] = -abs(X1[11, 2])
    p["X1"], p["X2"] = X1.astype("f4"), X2.astype("f4")
    for a in (p["X1"].astype("f8"), p["X2"].astype("f8")):                  # the equal steps survived the rounding to float32
        assert (a[7] - a[6] == a[8] - a[7]).all() and (a[7] != a[6]).any()
    p["max_err1"][12] = 0.0; p["max_err2"][13] = np.inf; p["max_err1"][14] = np.nan
    draws = make_draws(rng, [SPECIAL_N], SPECIAL_MAX_ITS)
    draws[0, :3] = [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    draws[0, 3:9] = corner_draws(SPECIAL_N)
    return p, draws


def _front_cloud(rng, n):
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2.5, 9, n)], 1).astype("f4")


def identity(fix_scale, seed=45):
    """X1 = X2 bit for bit: zero rotation (every off-diagonal entry of the first row of N is 0), t = 0, s = 1"""
    rng = np.random.default_rng(seed)
    p = ref.make_solver_problem(rng, SPECIAL_N, 0.0, fix_scale)
    p["X2"] = _front_cloud(rng, SPECIAL_N); p["X1"] = p["X2"].copy(); p["bad"][:] = False
    draws = make_draws(rng, [SPECIAL_N], SPECIAL_MAX_ITS)
    draws[0, :6] = corner_draws(SPECIAL_N)
    return p, draws


HALF_TURN_T0 = np.array([0.25, -0.5, 1.5], "f4")


def half_turn(seed=46):
    """X1 = diag(-1, -1, 1) X2 + t0: a rotation by 180 degrees about z (quaternion w = 0), z unchanged up to t0, so every point stays in
    front of both cameras.  The sum is rounded to float32 once; scale free."""
    rng = np.random.default_rng(seed)
    p = ref.make_solver_problem(rng, SPECIAL_N, 0.0, False)
    p["X2"] = _front_cloud(rng, SPECIAL_N)
    p["X1"] = (p["X2"].astype("f8") * [-1.0, -1.0, 1.0] + HALF_TURN_T0).astype("f4"); p["bad"][:] = False
    assert (p["X1"][:, 2] > 2).all() and (p["X2"][:, 2] > 2).all()
    draws = make_draws(rng, [SPECIAL_N], SPECIAL_MAX_ITS)
    draws[0, :6] = corner_draws(SPECIAL_N)
    return p, draws


def non_collinear(p, samples, rel=1e-2):
    """samples whose three points span a triangle in both frames: the smaller height is at least rel of the longest side (float64)"""
    out = np.ones(len(samples), bool)
    for X in (p["X1"].astype("f8"), p["X2"].astype("f8")):
        P = X[samples]
        a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        side = np.maximum(np.maximum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)), np.linalg.norm(a - b, axis=1))
        out &= np.linalg.norm(np.cross(a, b), axis=1) >= rel * side * side
    return out
