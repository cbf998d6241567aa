"""k_fast_cells scores one polarity per pass, chosen by a pixel's four compass pixels, and pushes a pixel with both compass flags
back on the wave's stack for a second pass (csrc/orb_fast_cells.hip).  Inputs on which that matters: corners on both-flag
pixels, bands in which most survivors are both-flag pixels (nearly every pop is pushed back: the stack bound and the tail loop),
a band whose scored-pixel list overflows, scores of 6 / 7 and 19 / 20 at the two thresholds.  Every case extracts a 2-frame batch
-- the frame and its inversion 255 - img, which swaps the polarities -- at 182 x 96 with 2 levels and compares, per frame and
level, the FAST candidates, and the keypoints and descriptors, with the CPU oracle.  The stated property of each input is
asserted on the input first.  The inversion has the original's level-0 candidates and scores; level 1 is a resampled image, whose
rounding is not symmetric under inversion, and is held to the oracle alone."""
import numpy as np
import pytest

from motioncheck_ccm_slam_amd.orb import ORBextractor

pytestmark = pytest.mark.gpu

NF, SF, INI, MN = 300, 1.2, 20, 7
W, H, NL = 182, 96, 2
BORDER = 16                                   # candidate coordinates are relative to the detection area's corner (19 - 3)


def _check(ctx, oracle, frames, nlevels, stride=None, offset=0):
    """frames [2, h, w] placed on the device with rows `stride` apart, the first `offset` bytes into a 16-byte-aligned buffer
    (default stride: w rounded up to 4); candidates of every level, keypoints and descriptors against the oracle.  Returns the
    extractor's level-0 candidates per frame."""
    import torch
    n, h, w = frames.shape
    stride = (w + 3) & ~3 if stride is None else stride
    plane = stride * h + 64
    host = np.random.default_rng(w * 1000 + h).integers(0, 256, offset + plane * n + 4096, dtype=np.uint8)
    for f in range(n):
        np.lib.stride_tricks.as_strided(host[offset + f * plane:], shape=(h, w), strides=(stride, 1))[...] = frames[f]
    buf = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    ex = ORBextractor(NF, SF, nlevels, INI, MN, ctx=ctx)
    ex.extract_dev(buf.data_ptr() + offset, w, h, stride, plane, n)
    kps, desc, counts = ex.fetch()
    par = oracle.default_params(NF, SF, nlevels, INI, MN)
    level0 = []
    for f in range(n):
        for l in range(nlevels):
            r = oracle.orb_extract(par, frames[f], cand_level=l)
            xy, sc = ex.fast_candidates(f, l)
            assert len(xy) == len(r["cand_xy"]) and (xy == r["cand_xy"]).all() and (sc == r["cand_score"]).all(), (f, l)
            if l == 0:
                level0.append((xy.copy(), sc.copy()))
        c = int(counts[f])
        assert c == len(r["kps"]), f
        for name in kps.dtype.names:
            assert (kps[f, :c][name] == r["kps"][name]).all(), (f, name)
        assert (desc[f, :c] == r["desc"]).all(), f
    del buf
    return level0


def _compass_flags(img, t):
    """Per pixel: the brighter / the darker polarity is possible at threshold t by the four compass pixels of the ring."""
    a = img.astype(np.int32)
    h, w = a.shape
    v = a[3:h - 3, 3:w - 3]
    n, s, e, wst = a[6:h, 3:w - 3], a[0:h - 6, 3:w - 3], a[3:h - 3, 6:w], a[3:h - 3, 0:w - 6]
    cb = np.zeros((h, w), bool)
    cd = np.zeros((h, w), bool)
    cb[3:h - 3, 3:w - 3] = np.minimum(np.maximum(n, s), np.maximum(e, wst)) > v + t
    cd[3:h - 3, 3:w - 3] = np.maximum(np.minimum(n, s), np.minimum(e, wst)) < v - t
    return cb, cd


def _figures(oracle, img):
    """Level 0: (candidates, candidates on both-flag pixels, survivors of the rejection test, both-flag survivors) in the
    detection area."""
    cb, cd = _compass_flags(img, min(INI, MN))
    det = np.zeros(img.shape, bool)
    det[19:img.shape[0] - 19, 19:img.shape[1] - 19] = True
    r = oracle.orb_extract(oracle.default_params(NF, SF, NL, INI, MN), img, cand_level=0)
    xy = r["cand_xy"]
    both = cb & cd & det
    return len(xy), int(both[xy[:, 1] + BORDER, xy[:, 0] + BORDER].sum()), int(((cb | cd) & det).sum()), int(both.sum())


def _run_with_inversion(ctx, oracle, img):
    lv0 = _check(ctx, oracle, np.stack([img, 255 - img]), NL)
    assert (lv0[0][0] == lv0[1][0]).all() and (lv0[0][1] == lv0[1][1]).all()
    return lv0[0]


def _band_segment_test_count(img):
    """Pixels of the first band's detection rectangle (x 19..138, y 19..(19 + cell height - 1)) that pass the segment test at
    minThFAST: more than FC_NZ = 1024 overflow the band's list of scored pixels."""
    ring = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
    a = img.astype(np.int32)
    h, w = a.shape
    v = a[3:h - 3, 3:w - 3]
    r = np.stack([a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in ring])
    out = np.zeros((h, w), bool)
    for m in (r > v + MN, r < v - MN):
        m2 = np.concatenate([m, m[:8]])
        out[3:h - 3, 3:w - 3] |= np.any([np.all(m2[k:k + 9], axis=0) for k in range(16)], axis=0)
    hcell = -(-(h - 32) // ((h - 32) // 30))
    return int(out[19:19 + hcell, 19:139].sum())


@pytest.mark.parametrize("frame", [0, 1])
def test_uniform_noise(ctx, oracle, frame):
    """850 / 853 level-0 candidates, 13 / 8 of them on both-flag pixels; the first band's scored-pixel list overflows."""
    img = np.random.default_rng(5).integers(0, 256, (2, H, W), dtype=np.uint8)[frame]
    ncand, on_both, _, _ = _figures(oracle, img)
    assert ncand >= 800 and on_both >= 5
    assert _band_segment_test_count(img) > 1024
    xy, _ = _run_with_inversion(ctx, oracle, img)
    assert len(xy) == ncand


def test_ramp_with_noise(ctx, oracle):
    """484 candidates, 9 on both-flag pixels, 595 both-flag survivors on level 0."""
    y, x = np.indices((H, W))
    img = np.clip((3 * (x + y)) % 200 + 20 + np.random.default_rng(9).integers(-40, 41, (H, W)), 0, 255).astype(np.uint8)
    ncand, on_both, _, both = _figures(oracle, img)
    assert on_both >= 5 and both >= 500
    xy, _ = _run_with_inversion(ctx, oracle, img)
    assert len(xy) == ncand


def test_ramp_with_two_rectangles(ctx, oracle):
    """8,234 survivors on level 0, 7,233 of them both-flag, 2 candidates: nearly every pop is pushed back."""
    y, x = np.indices((H, W))
    img = (3 * (x + y)) % 256
    img[30:44, 40:60] += 90
    img[50:64, 100:120] -= 90
    img = np.clip(img, 0, 255).astype(np.uint8)
    ncand, _, surv, both = _figures(oracle, img)
    assert surv > 5000 and both >= 0.8 * surv
    xy, _ = _run_with_inversion(ctx, oracle, img)
    assert len(xy) == ncand == 2


def test_isolated_pixels(ctx, oracle):
    """Single pixels 7, 8, 20, 21 above and below a flat 100: score 6 against 7 at minThFAST, and a score of 19 dropped in a
    cell that holds a score of 20 (iniThFAST)."""
    img = np.full((H, W), 100, np.uint8)
    for i, p in enumerate((107, 108, 120, 121, 92, 93, 80, 79)):
        img[40, 30 + 15 * i] = p
    r = oracle.orb_extract(oracle.default_params(NF, SF, NL, INI, MN), img, cand_level=0)
    assert r["cand_xy"].tolist() == [[29, 24], [59, 24], [74, 24], [119, 24]] and r["cand_score"].tolist() == [7, 20, 7, 20]
    xy, sc = _run_with_inversion(ctx, oracle, img)
    assert xy.tolist() == [[29, 24], [59, 24], [74, 24], [119, 24]] and sc.tolist() == [7, 20, 7, 20]
