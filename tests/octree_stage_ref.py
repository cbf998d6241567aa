"""Stage check of k_octree on the GPU's own input (used by test_octree_stage_gpu.py and by its child processes).

For every (frame, level) the FAST candidates the kernel gathered are taken from the debug tap (ccm_orb_debug_candidates: xy relative
to the 16 px border, scores, cell-major order), the oracle's orc_distribute_octree runs on exactly those with the level's bounds and
quota as orb_oracle.c's operator() forms them, and the keys it selects, in its order, must be the keypoints the extractor returned
for that octave: x, y (scaled back as the reference does) and response equal, and the same number of them.  Whatever FAST or the
pyramid did, the quadtree is held to its own input."""
import ctypes as C

import numpy as np

from motioncheck_ccm_slam_amd import synth
from orb_definitions_ref import BORDER, CELL, EDGE

OCT_LDS_KEYS = 2048          # csrc/orb_octree.hip: candidates of a level up to which the keys stay in LDS and registers
GATHER_ROUND = 256           # cells a round of the kernel's loop gather takes
DENSE_SEED, DENSE_BLOCK = 0, 2      # chosen on the CPU with the oracle's candidate output: at 320x240 level 1 brings 2,444 candidates, a cell of level 0 holds 29


def frame_a():
    """the first bench frame, 752x480"""
    return synth.frames(0, 1)[0]


def dense_frame(w, h, seed=DENSE_SEED, block=DENSE_BLOCK):
    """seeded binary blocks of `block` pixels: a FAST corner at most block junctions"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, ((h + block - 1) // block, (w + block - 1) // block), dtype=np.uint8)
    return (np.kron(bits, np.ones((block, block), np.uint8))[:h, :w] * 190 + 30).astype(np.uint8)


def blank_frame(w, h):
    return np.full((h, w), 90, np.uint8)


def one_corner_frame(w, h):
    """one bright quadrant corner in the middle of a dark frame: a single candidate on level 0"""
    img = np.full((h, w), 30, np.uint8)
    img[h // 2:, w // 2:] = 220
    return img


def cell_grid(lw, lh):
    """(nCols, nRows, wCell, hCell) of a level, ORBextractor.cpp:941-956"""
    width, height = np.float32(lw - 2 * BORDER), np.float32(lh - 2 * BORDER)
    ncols, nrows = int(width / np.float32(CELL)), int(height / np.float32(CELL))
    if ncols < 1 or nrows < 1:
        return 0, 0, 1, 1
    return ncols, nrows, int(np.ceil(width / np.float32(ncols))), int(np.ceil(height / np.float32(nrows)))


def cell_counts(xy, lw, lh):
    """candidates per FAST cell from their coordinates: cell (i, j) detects the border-relative pixels [3 + j wCell, 3 + (j + 1) wCell)
    x [3 + i hCell, ...), the last column and row up to the border.  Also checks that the tap's order is cell-major."""
    ncols, nrows, wc, hc = cell_grid(lw, lh)
    if len(xy) == 0:
        return np.zeros(max(ncols * nrows, 1), np.int64)
    j = np.minimum((xy[:, 0] - 3) // wc, ncols - 1); i = np.minimum((xy[:, 1] - 3) // hc, nrows - 1)
    ci = i * ncols + j
    assert (np.diff(ci) >= 0).all(), "candidates are not in cell-major order"
    return np.bincount(ci, minlength=ncols * nrows)


def check_stage(ex, oracle, par, kps, counts, w, h, frames=None):
    """ex: the extractor after a call on frames of w x h; kps, counts: what it returned.  Returns {(frame, level): dict(n=candidates,
    selected=keypoints, quota=, cells=, max_cell=)} for the preconditions the cases assert."""
    lw, lh = ex.level_sizes(w, h)
    olw, olh = oracle.level_sizes(par, w, h)
    assert (lw == olw).all() and (lh == olh).all()
    tab = oracle.orb_tables(par)
    quota, scale = tab["nfeat"], tab["scale"]
    info = {}
    for f in (range(len(counts)) if frames is None else frames):
        k = kps[f, :counts[f]]
        assert (np.diff(k["octave"]) >= 0).all()
        for l in range(par.nlevels):
            xy, sc = ex.fast_candidates(f, l)
            xy = np.ascontiguousarray(xy, "i4"); sc = np.ascontiguousarray(sc, "i4")
            sel = np.zeros(len(xy) + 8, "i4")
            # bounds and quota of the level: oracle/orb_oracle.c:571-572 and :608
            ns = oracle.lib().orc_distribute_octree(xy.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), len(xy),
                                                    EDGE - 3, int(lw[l]) - EDGE + 3, EDGE - 3, int(lh[l]) - EDGE + 3, int(quota[l]),
                                                    sel.ctypes.data_as(C.c_void_p))
            assert ns >= 0
            sel = sel[:ns]
            got = k[k["octave"] == l]
            assert len(got) == ns, "frame %d level %d: %d keypoints, the oracle's tree selects %d of %d candidates" % (f, l, len(got), ns, len(xy))
            # :1012-1013 and :1268-1274: border added, then scaled back in float unless level 0
            ex_x = (xy[sel, 0] + (EDGE - 3)).astype(np.float32); ex_y = (xy[sel, 1] + (EDGE - 3)).astype(np.float32)
            if l != 0:
                ex_x = ex_x * np.float32(scale[l]); ex_y = ex_y * np.float32(scale[l])
            assert (got["x"] == ex_x).all() and (got["y"] == ex_y).all(), "frame %d level %d: keys or their order differ" % (f, l)
            assert (got["response"] == sc[sel].astype(np.float32)).all(), "frame %d level %d: responses differ" % (f, l)
            cc = cell_counts(xy, int(lw[l]), int(lh[l]))
            info[(f, l)] = dict(n=len(xy), selected=ns, quota=int(quota[l]), cells=len(cc), max_cell=int(cc.max()) if len(cc) else 0)
    return info
