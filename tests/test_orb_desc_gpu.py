"""Descriptor kernel (k_orient_desc) against the CPU oracle, descriptor for descriptor: keypoints whose 43x43 patch crosses
an image edge at every pyramid level (the BORDER_REFLECT_101 patch path), in a single-frame call (one keypoint per wave) and
inside a batch large enough for the looping form (eight keypoint slots per wave).  The column blur is evaluated at the
rotated sample points only, so the checked keypoints must cover every angle quadrant and both row parities of those points."""
import os
import re

import numpy as np
import pytest

from motioncheck_ccm_slam_amd import synth
from motioncheck_ccm_slam_amd.orb import ORBextractor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 752, 480
# k_orient_desc takes the one-slot-per-wave form below 4 * 8192 keypoint slots per launch; a frame has ~1,000 slots with
# these parameters, so 48 frames are well inside the looping form and one frame well inside the other
BATCH = 48


def _pattern():
    with open(os.path.join(ROOT, "include", "ccm_orb_pattern.h")) as fh:
        body = fh.read().split("{", 1)[1].split("}", 1)[0]
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], np.float32).reshape(512, 2)


def _edge_frame(seed):
    """Noise in a 96-pixel frame along every edge (27 pixels on level 7), flat inside: keypoints only near the edges."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W), dtype=np.uint8)
    img[96:H - 96, 96:W - 96] = 128
    return img


def _same(kps, desc, ref, what):
    assert len(kps) == len(ref["kps"]), what
    for name in kps.dtype.names:
        assert (kps[name] == ref["kps"][name]).all(), (what, name)
    bad = np.nonzero((desc != ref["desc"]).any(1))[0]
    assert len(bad) == 0, (what, "descriptor rows differ", bad[:10])


def _coverage(ex, kps):
    """The angle quadrants and sample-row parities the keypoints exercise, and how many sit within 21 px of an edge per level."""
    sc = np.asarray(ex.GetScaleFactors(), np.float32)
    lw, lh = ex.level_sizes(W, H)
    o = kps["octave"]
    x = kps["x"] / sc[o]; y = kps["y"] / sc[o]
    near = (x < 21) | (y < 21) | (x > lw[o] - 1 - 21) | (y > lh[o] - 1 - 21)
    near_per_level = np.bincount(o[near], minlength=8)
    quadrants = set((kps["angle"] // 90).astype(int).tolist())
    p = _pattern()
    t = np.deg2rad(kps["angle"].astype(np.float64))
    a, b = np.cos(t).astype(np.float32), np.sin(t).astype(np.float32)
    dy = np.rint(p[None, :, 0] * b[:, None] + p[None, :, 1] * a[:, None]).astype(int)
    return near_per_level, quadrants, set((dy & 1).ravel().tolist())


def test_edge_keypoints_single_frame(ctx, oracle):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    par = oracle.default_params()
    for seed in (0, 1):
        img = _edge_frame(seed)
        kps, desc = ex(img)
        _same(kps, desc, oracle.orb_extract(par, img), ("single", seed))
        near, quadrants, parities = _coverage(ex, kps)
        assert (near > 0).all(), near
        assert quadrants == {0, 1, 2, 3} and parities == {0, 1}


def test_edge_keypoints_in_batch(ctx, oracle):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    par = oracle.default_params()
    imgs = synth.frames(7, BATCH)
    imgs[0] = _edge_frame(0)
    imgs[BATCH // 2] = _edge_frame(1)
    imgs[BATCH - 1] = _edge_frame(2)
    kps, desc, counts = ex.extract_batch(imgs)
    for f in range(BATCH):
        n = int(counts[f])
        _same(kps[f, :n], desc[f, :n], oracle.orb_extract(par, imgs[f]), ("batch", f))
    for f in (0, BATCH // 2, BATCH - 1):
        n = int(counts[f])
        near, quadrants, parities = _coverage(ex, kps[f, :n])
        assert (near > 0).all(), (f, near)
        assert quadrants == {0, 1, 2, 3} and parities == {0, 1}
        # the same frame alone (one keypoint slot per wave) gives the same rows
        k1, d1 = ex(imgs[f])
        assert (k1 == kps[f, :n]).all() and (d1 == desc[f, :n]).all(), f
