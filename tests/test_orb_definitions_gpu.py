"""The HIP extractor's stages against tests/orb_definitions_ref.py, the published definitions restated in numpy: no oracle in between.
Stage outputs come through the extractor's own taps (image_pyramid_level, fast_candidates) and its results.  Every stage is checked
on the GPU's own input to that stage, so one stage's error is not charged to the next.  The quadtree is not restated: the tests hold
it to the properties that any faithful DistributeOctTree has.

Cases (shapes chosen for where the kernels can go wrong, not for the workload):
  A        233x171 synthetic, 4 levels: odd widths at every level (233, 194, 162, 135), tail rows of the resize's row blocks
  B        as A on uniform noise: ~130 maxima and ~310 scored pixels per cell, every NMS tie rule
  B_low    as B with both thresholds at 7: more than 1024 scored pixels in three adjacent cells, past the band's list of scored pixels
  C_*      the skipped last cell column (813 wide) and row (903 high), a grid one cell row high and one a single cell column wide.
           The 813x97 and 97x903 strips of the CPU test give 12 and 0 quadtree roots, which the library refuses (1..8 supported, and
           the reference divides by zero at 0); these are the narrowest images of those lengths that it accepts at both levels
  D_*      200x160 with ini=7, min=20 and ini=60, min=7: the fallback threshold taken in most cells, or never
  E        as A with 60 features: the quadtree prunes
  F        image 2 of a batch of three different 233x171 frames: per-image offsets
"""
import numpy as np
import pytest

import orb_definitions_ref as D
from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.orb import ORBextractor

pytestmark = pytest.mark.gpu

AMBIGUOUS_CAP = 0.005          # share of a case's BRIEF bits that may be set aside as rounding-ambiguous


def _noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


# name: (images [B,H,W] maker, image checked, (nfeatures, scale, nlevels, ini, min))
CASES = {
    "A": (lambda: synth.frame(5, 233, 171)[None], 0, (300, 1.2, 4, 20, 7)),
    "B": (lambda: _noise(2, 233, 171)[None], 0, (300, 1.2, 4, 20, 7)),
    "B_low": (lambda: _noise(2, 233, 171)[None], 0, (300, 1.2, 4, 7, 7)),
    "C_skipped_column": (lambda: synth.frame(7, 813, 131, n_rect=150)[None], 0, (300, 1.2, 2, 20, 7)),
    "C_skipped_row": (lambda: synth.frame(8, 480, 903, n_rect=500)[None], 0, (300, 1.2, 2, 20, 7)),
    "C_one_cell_row": (lambda: synth.frame(9, 400, 90, n_rect=60)[None], 0, (300, 1.2, 2, 20, 7)),
    "C_one_cell_column": (lambda: synth.frame(13, 90, 140, n_rect=60)[None], 0, (300, 1.2, 2, 20, 7)),
    "D_ini7_min20": (lambda: synth.frame(3, 200, 160)[None], 0, (300, 1.2, 4, 7, 20)),
    "D_ini60_min7": (lambda: synth.frame(3, 200, 160)[None], 0, (300, 1.2, 4, 60, 7)),
    "E": (lambda: synth.frame(5, 233, 171)[None], 0, (60, 1.2, 4, 20, 7)),
    "F": (lambda: synth.frames(5, 3, 233, 171), 2, (300, 1.2, 4, 20, 7)),
}


class Run:
    """One extraction and everything the tests need from it, taken at once: the taps read the context's last extraction."""

    def __init__(self, ctx, name):
        make, f, par = CASES[name]
        self.name, self.par = name, par
        nfeat, sf, nl, ini, mn = par
        ex = ORBextractor(nfeat, sf, nl, ini, mn, ctx=ctx)
        imgs = make()
        kps, desc, counts = ex.extract_batch(imgs)
        self.image = imgs[f]
        self.kps = kps[f, :counts[f]].copy()
        self.bits = np.unpackbits(desc[f, :counts[f]], axis=1, bitorder="little")
        assert (kps[f, counts[f]:]["size"] == 0).all()
        self.levels = [ex.image_pyramid_level(f, l) for l in range(nl)]
        self.cand = [ex.fast_candidates(f, l) for l in range(nl)]
        self.quota = ex.mnFeaturesPerLevel.copy()
        self.scale = ex.GetScaleFactors()
        # level coordinates of the keypoints: pt was multiplied by mvScaleFactor[level] at the end (ORBextractor.cpp:1268-1274)
        l = self.kps["octave"]
        self.fx = self.kps["x"].astype(np.float64) / self.scale[l]; self.fy = self.kps["y"].astype(np.float64) / self.scale[l]
        self.x = np.rint(self.fx).astype(int); self.y = np.rint(self.fy).astype(int)


@pytest.fixture(scope="module", params=list(CASES))
def run(request, ctx):
    return Run(ctx, request.param)


def _cells_across(n):
    """nCols or nRows of a level n pixels across (ORBextractor.cpp:941-953)."""
    return int((n - 2 * D.EDGE + 6) / D.CELL)


def test_pyramid(run):
    nfeat, sf, nl, ini, mn = run.par
    h, w = run.image.shape
    lw, lh = D.level_sizes(w, h, sf, nl)
    if run.name == "A":
        assert lw == [233, 194, 162, 135]
    assert [lev.shape for lev in run.levels] == list(zip(lh, lw))
    assert (run.levels[0] == run.image).all()
    worst = 0.0
    for l in range(1, nl):
        # one of the two integers that bracket the float64 bilinear value of the GPU's own previous level
        dev = np.abs(run.levels[l].astype(np.float64) - D.resize(run.levels[l - 1], lw[l], lh[l])).max()
        worst = max(worst, dev)
        assert dev < 1.0, (l, dev)
    print("%s: worst resize deviation %.3f" % (run.name, worst))


def test_candidates(run):
    nfeat, sf, nl, ini, mn = run.par
    skipped = [0, 0]
    for l in range(nl):
        dxy, dsc, skip_c, skip_r = D.cell_candidates(run.levels[l], ini, mn)
        xy, sc = run.cand[l]
        assert len(dxy) > 0, l
        got = sorted(zip(xy[:, 0].tolist(), xy[:, 1].tolist(), sc.tolist()))
        want = sorted(zip(dxy[:, 0].tolist(), dxy[:, 1].tolist(), dsc.tolist()))
        assert got == want, "level %d: %d candidates, the definition gives %d" % (l, len(got), len(want))
        assert (xy == dxy).all() and (sc == dsc).all(), "level %d: same candidates in another order" % l       # row-major in a cell, cells row-major
        skipped[0] += skip_c; skipped[1] += skip_r
        if l == 0:
            if run.name == "C_one_cell_row":
                assert _cells_across(run.levels[0].shape[0]) == 1
            if run.name == "C_one_cell_column":
                assert _cells_across(run.levels[0].shape[1]) == 1
            if run.name == "B_low":
                # the first three cells of the top cell row hold more scored pixels than the kernel's list of them (FC_NZ = 1024)
                s = D.fast_score_map(run.levels[0][16:16 + 36, 16:16 + 3 * 34 + 6])
                assert (s >= ini).sum() > 1024
    print("%s: %s candidates, %d cell columns and %d cell rows skipped" % (run.name, [len(c[1]) for c in run.cand], skipped[0], skipped[1]))
    if run.name == "C_skipped_column":
        assert skipped[0] > 0
    if run.name == "C_skipped_row":
        assert skipped[1] > 0
    if run.name in ("D_ini7_min20", "D_ini60_min7"):
        # a cell that is empty at 7 is empty at 20, so min=20 adds nothing; at ini=60 most cells are empty and fall back to 7
        alone = D.cell_candidates(run.levels[0], ini, ini)
        assert (len(alone[0]) != len(run.cand[0][0])) == (ini > mn)


def test_keypoints_and_quadtree_properties(run):
    """The lower bound on a level's count, min(quota, candidates), holds on these inputs and not on every input: DistributeOctTree
    stops when a pass leaves the number of nodes unchanged (ORBextractor.cpp:837), which a level of a dozen candidates with two of
    them close together can reach with both still in one node.  The one-cell-column frame was chosen to have no such level."""
    nfeat, sf, nl, ini, mn = run.par
    k = run.kps
    assert len(k) > 0 and (np.diff(k["octave"]) >= 0).all()                      # level-major
    assert (k["octave"] >= 0).all() and (k["octave"] < nl).all()
    assert np.abs(run.fx - run.x).max() < 1e-3 and np.abs(run.fy - run.y).max() < 1e-3
    # keypoints[i].size = scaledPatchSize, an int: PATCH_SIZE*mvScaleFactor[level] truncated (ORBextractor.cpp:1006, 1015)
    assert (k["size"] == np.floor(np.float32(31) * run.scale[k["octave"]])).all()
    if run.name in ("A", "B"):
        assert len(k) % 8 != 0       # neither whole waves (8 keypoints) nor whole workgroups (32) in k_orient_desc
    per = np.bincount(k["octave"], minlength=nl)
    pruned = False
    for l in range(nl):
        xy, sc = run.cand[l]
        score = {(int(x), int(y)): int(s) for (x, y), s in zip(xy, sc)}
        sel = k["octave"] == l
        kept = list(zip((run.x[sel] - D.BORDER).tolist(), (run.y[sel] - D.BORDER).tolist()))
        assert len(set(kept)) == len(kept)
        for p, r in zip(kept, k["response"][sel]):
            assert p in score and score[p] == r, (l, p, r)
        assert min(run.quota[l], len(sc)) <= per[l] <= run.quota[l] + 3, (l, per[l], run.quota[l], len(sc))
        if (sc == sc.max()).sum() == 1:
            assert tuple(xy[sc.argmax()]) in kept, l
        pruned |= per[l] < len(sc)
    print("%s: kept %s of %s candidates, quotas %s" % (run.name, per.tolist(), [len(c[1]) for c in run.cand], run.quota.tolist()))
    if run.name == "E":
        assert pruned


def test_angles(run):
    """Bound: the worst error of fastAtan2's published polynomial against float64 atan, 0.00955 degrees, plus 1e-3 for float32: 0.01055."""
    bound = D.angle_bound()
    k = run.kps
    assert (k["angle"] >= 0).all() and (k["angle"] < 360).all()
    ref = np.array([D.ic_angle(run.levels[l], x, y) for l, x, y in zip(k["octave"], run.x, run.y)])
    err = D.angle_diff(k["angle"], ref)
    print("%s: worst angle error %.5f of %.5f over %d keypoints" % (run.name, err.max(), bound, len(k)))
    assert err.max() <= bound, (int(err.argmax()), err.max())


def test_descriptors(run):
    k = run.kps
    blurred = [D.blur(lev) for lev in run.levels]
    wrong = amb_n = 0
    for i in range(len(k)):
        bits, amb = D.brief(blurred[k["octave"][i]], run.x[i], run.y[i], float(k["angle"][i]))
        wrong += int(((bits != run.bits[i]) & ~amb).sum()); amb_n += int(amb.sum())
    total = 256 * len(k)
    print("%s: %d bits, %d ambiguous (%.3f %%), %d wrong" % (run.name, total, amb_n, 100.0 * amb_n / total, wrong))
    assert amb_n <= AMBIGUOUS_CAP * total
    assert wrong == 0


@pytest.mark.parametrize("w,h", [(813, 97), (97, 903)])
def test_strips_outside_the_quadtree_range_are_refused(ctx, w, h):
    """12 and 0 quadtree roots: refused before any launch, as an error and not as a fault."""
    ex = ORBextractor(300, 1.2, 2, 20, 7, ctx=ctx)
    with pytest.raises(_lib.CcmError):
        ex(synth.frame(7, w, h, n_rect=120))
