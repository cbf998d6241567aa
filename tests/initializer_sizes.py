"""Two-view scenes past one LDS tile of k_init_hypotheses (INI_TILE = 1024 matches), shared by tests/test_initializer_sizes_cpu.py and
tests/test_initializer_sizes_gpu.py.  initializer_ref.CASES stays as it is: the committed tolerances were measured on it.

Nine sets are one workgroup's eight plus one, seventeen two plus one.  Random sets of eight are almost all contaminated at these
wrong-match shares, so the first rows are planted: sets drawn wholly from correct matches, the first of them holding the last match
(the only one of the last tile at N = 1025 and 2049)."""
import numpy as np

import initializer_ref as ref

TILE, SPB = 1024, 8                                    # INI_TILE, INI_SPB (csrc/init_types.h)
#             N, wrong-match share, kind, sets
SIZE_CASES = [(1023, 0.3, "general", 9), (1024, 0.2, "plane", 9), (1025, 0.3, "general", 9), (2049, 0.3, "plane", 9), (2049, 0.3, "general", 17)]
SEED = 57
PLANTED = 4
PLANE_2049 = 3                                         # the case whose chosen mask spans 33 words in k_init_check_rt


def correct_sets(rng, p, n, count):
    """`count` rows of draws that select eight correct matches each; row 0 holds match n - 1.  Below n - 8 a draw selects the index it
    names (no swapped-in element), so distinct values there are the set itself."""
    good = np.flatnonzero(~p["wrong"])
    assert not p["wrong"][n - 1], "the seed must leave the last match a correct one"
    low = good[good < n - 8]
    rows = []
    for k in range(count):
        row = rng.choice(low, 8, replace=False)
        if k == 0:
            row[0] = n - 1
        assert (ref.sample_sets(n, row)[0] == row).all()
        rows.append(row)
    return np.array(rows, "i4")


def make_size_cases(seed=SEED):
    """[(problem, draws [sets][8])] for SIZE_CASES"""
    rng = np.random.default_rng(seed)
    out = []
    for n, share, kind, its in SIZE_CASES:
        p = ref.make_two_view(rng, n, share, kind)
        hi = np.maximum(n - np.arange(8), 1)
        d = rng.integers(0, np.broadcast_to(hi, (its, 8))).astype("i4")
        d[:PLANTED] = correct_sets(rng, p, n, PLANTED)
        d[PLANTED] = n - 1 - np.arange(8)               # the last index each time
        d[PLANTED + 1] = 0                              # index 0 each time: positions 0 takes the last element
        out.append((p, d))
    return out


def tiles_populated(mask):
    """per tile of 1024 matches: does the mask [N] hold an inlier there"""
    return [bool(mask[t0:t0 + TILE].any()) for t0 in range(0, len(mask), TILE)]
