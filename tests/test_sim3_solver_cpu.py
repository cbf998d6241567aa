"""Batched Sim3Solver, the parts that need no device: SetRansacParameters' iteration count as the library exports it, the
reference class the GPU tests use as their yardstick (tests/sim3_solver_ref.py) against hand-made count sequences, and the
binding's symbol list."""
import math

import numpy as np

from motioncheck_ccm_slam_amd import _lib
import sim3_solver_ref as ref


def _formula(n, p, min_inliers, cap):
    """src/Sim3Solver.cpp:100-115 as the header states it; 1 where the reference's expression is undefined (n < min_inliers)."""
    if n < min_inliers:
        return 1
    if min_inliers == n:
        it = 1
    else:
        eps = float(np.float32(min_inliers) / np.float32(n))
        den = math.log(1 - eps ** 3)
        # den = 0 (min_inliers = 0): the quotient is -inf, (int)ceil(-inf) is out of int's range and :115's max(1, ...) clamps what
        # compilers make of it; the definition is 1
        it = math.ceil(math.log(1 - p) / den) if den != 0 else 1
    return max(1, min(it, cap))


def test_ransac_iterations_matches_set_ransac_parameters():
    f = _lib.load().ccm_sim3_ransac_iterations
    for n in range(3, 401):
        for mi in (0, 1, 3, 6, 20):
            for p in (0.99, 0.999):
                for cap in (300, 50):
                    assert f(n, p, mi, cap) == _formula(n, p, mi, cap) == ref.ransac_iterations(n, p, mi, cap), (n, mi, p, cap)
    for n in (3, 70, 400):                                # MinInliers 0: log(1 - 0) = 0, one iteration whatever the cap
        assert f(n, 0.99, 0, 300) == ref.ransac_iterations(n, 0.99, 0, 300) == 1
    for (n, mi), want in {(3, 1): 123, (4, 1): 210, (7, 1): 210, (3, 3): 1, (4, 3): 9, (70, 3): 210}.items():
        assert f(n, 0.99, mi, 210) == want, (n, mi)
    for (n, mi), want in {(6, 6): 1, (7, 6): 5, (8, 6): 9, (20, 6): 169, (25, 20): 7, (100, 6): 300}.items():
        assert f(n, 0.99, mi, 300) == want, (n, mi)
    for n, mi in ((5, 6), (0, 6), (19, 20), (3, 20)):
        assert f(n, 0.99, mi, 300) == 1


def test_reference_class_follows_iterate():
    idx = np.array([1, 3, 4, 6, 7, 9, 10, 12, 13, 15])
    counts = [3, 6, 6, 5, 7, 7, 9, 2]
    masks = np.zeros((8, 10), bool)
    for h, c in enumerate(counts):
        masks[h, (np.arange(c) + h) % 10] = True
    s = ref.RefSolver(10, 16, idx, counts, masks, min_inliers=6, max_its=8)
    h, no_more, vb, n = s.iterate(1)                       # 3 >= 0: the best, but no return
    assert (h, no_more, n, s.best, s.mnBestInliers, s.mnIterations) == (None, False, 0, 0, 3, 1) and not vb.any() and len(vb) == 16
    h, no_more, vb, n = s.iterate(2)                       # 6 > 6 is false (strict); the second 6 replaces the first (>=)
    assert (h, no_more, n, s.best, s.mnBestInliers, s.mnIterations) == (None, False, 0, 2, 6, 3)
    h, no_more, vb, n = s.iterate(5)                       # 5 < best; 7 returns after two of the five iterations
    assert (h, no_more, n, s.mnIterations) == (4, False, 7, 5)
    assert sorted(np.flatnonzero(vb)) == sorted(idx[masks[4]]) and vb.sum() == 7     # through mvnIndices1
    h, no_more, vb, n = s.iterate(5)                       # resumed: the per-call counter restarts, 7 >= 7 returns again
    assert (h, no_more, n, s.mnIterations) == (5, False, 7, 6)
    h, no_more, vb, n = s.iterate(1)
    assert (h, no_more, n, s.mnIterations) == (6, False, 9, 7)
    h, no_more, vb, n = s.iterate(5)                       # 2 < 9, then mnIterations reaches mRansacMaxIts without a return
    assert (h, no_more, n, s.mnIterations, s.best) == (None, True, 0, 8, 6) and not vb.any()
    assert s.iterate(5)[:2] == (None, True)
    # a return on the very last hypothesis does not set bNoMore; the next call does
    s = ref.RefSolver(10, 10, np.arange(10), [1, 1, 9], np.ones((3, 10), bool), 6, 3)
    h, no_more, vb, n = s.iterate(3)
    assert (h, no_more, n) == (2, False, 9)
    assert s.iterate(1)[:2] == (None, True)
    # find = iterate(mRansacMaxIts); a best below the bar is kept but not returned
    s = ref.RefSolver(10, 10, np.arange(10), [1, 6, 2], np.ones((3, 10), bool), 6, 3)
    h, vb, n = s.find()
    assert (h, n, s.best, s.mnBestInliers) == (None, 0, 1, 6)
    # N < minInliers: bNoMore and nothing else
    s = ref.RefSolver(5, 9, np.arange(5), [5, 5], np.ones((2, 5), bool), 6, 1)
    h, no_more, vb, n = s.iterate(5)
    assert (h, no_more, n, s.mnIterations, s.best) == (None, True, 0, 0, -1) and len(vb) == 9
    # mnBestInliers carried over a SetRansacParameters
    s = ref.RefSolver(10, 10, np.arange(10), [7, 8], np.ones((2, 10), bool), 6, 2, best_inliers=8)
    assert s.iterate(1)[0] is None and s.iterate(1)[0] == 1


def test_reference_sampling_is_swap_with_last():
    assert ref.sample_indices(10, [9, 8, 7]) == [9, 8, 7]          # the last element each time
    assert ref.sample_indices(10, [0, 0, 0]) == [0, 9, 8]          # position 0 takes the last element
    assert ref.sample_indices(10, [3, 3, 3]) == [3, 9, 8]
    assert ref.sample_indices(10, [8, 8, 0]) == [8, 9, 0]
    assert ref.sample_indices(3, [0, 1, 0]) == [0, 1, 2]


def test_binding_lists_the_solver_symbols():
    for name in ("ccm_sim3_ransac_iterations", "ccm_sim3_solver_create", "ccm_sim3_solver_destroy", "ccm_sim3_solver_iterate",
                 "ccm_sim3_solver_find", "ccm_sim3_solver_estimate", "ccm_sim3_solver_hypotheses"):
        assert name in _lib.SYMBOLS
    from motioncheck_ccm_slam_amd import sim3solver
    assert sim3solver.make_draws(np.random.default_rng(0), [10, 2, 0], 7).shape == (3, 7, 3)
