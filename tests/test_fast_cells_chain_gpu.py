"""k_fast_cells on the shapes at which its staging, NMS and rank loops take different paths: one, two and three staging
trips per thread, the row-end clamp at every width % 4, level-0 frames in caller layouts that select the 16-byte, dword
and byte staging, cells that fall back to minThFAST (their count comes from the per-cell counters), score ties, and
bands whose candidate lists overflow.  Every case extracts a 2-frame batch (frame index > 0) and compares, per frame, the
FAST candidates of every level and the keypoints and descriptors with the CPU oracle."""
import numpy as np
import pytest

from motioncheck_ccm_slam_amd import synth
from motioncheck_ccm_slam_amd.orb import ORBextractor

pytestmark = pytest.mark.gpu

NF, SF, INI, MN = 300, 1.2, 20, 7


def _pair(w, h, seed=7):
    return np.stack([synth.frame(seed + f, w, h, n_rect=max(60, 600 * w * h // (752 * 480))) for f in range(2)])


def _check(ctx, oracle, frames, nlevels, stride=None, offset=0):
    """frames [2, h, w] placed on the device with rows `stride` apart, the first `offset` bytes into a 16-byte-aligned buffer.
    Default stride: w rounded up to 4, so that with offset 0 every frame and row starts on a dword and level 0 (the caller's
    buffer, read in place) is staged 16 bytes per lane; a stride or a frame address that is no multiple of 4 selects the byte
    path for level 0.  The pyramid levels above are the library's own (pitch a multiple of 64): always 16 bytes per lane."""
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
    for f in range(n):
        for l in range(nlevels):
            r = oracle.orb_extract(par, frames[f], cand_level=l)
            xy, sc = ex.fast_candidates(f, l)
            assert len(xy) == len(r["cand_xy"]) and (xy == r["cand_xy"]).all() and (sc == r["cand_score"]).all(), (f, l)
        c = int(counts[f])
        assert c == len(r["kps"]), f
        for name in kps.dtype.names:
            assert (kps[f, :c][name] == r["kps"][name]).all(), (f, name)
        assert (desc[f, :c] == r["desc"]).all(), f
    del buf


def _cand0(oracle, img, nlevels):
    return oracle.orb_extract(oracle.default_params(NF, SF, nlevels, INI, MN), img, cand_level=0)["cand_score"]


@pytest.mark.parametrize("packed", [False, True], ids=["rows_on_dwords", "rows_packed"])
@pytest.mark.parametrize("w,h,nl", [
    (96, 96, 2),        # 2-cell bands of pitch 80: 190 16-byte items, one trip per thread, the fourth wave idle
    (182, 96, 3),       # a 4-cell and a 1-cell band per cell row: two trips
    (182, 91, 3),       # one cell row of height 59: 65 tile rows of pitch 144, 585 items, three trips (the largest band the reciprocals allow)
])
def test_staging_trips(ctx, oracle, w, h, nl, packed):
    """Level 0 with rows on dword boundaries (stride 184 for w = 182): the item counts above, 16 bytes per lane.  With
    packed rows (stride = w = 182) level 0 of the 182-wide cases takes the byte path instead: bh * pitch one-byte items."""
    _check(ctx, oracle, _pair(w, h), nl, stride=w if packed else None)


@pytest.mark.parametrize("packed", [False, True], ids=["rows_on_dwords", "rows_packed"])
@pytest.mark.parametrize("w", [181, 182, 183, 184])
def test_row_end_clamp(ctx, oracle, w, packed):
    """Every w % 4 on level 0 with rows on dword boundaries: the last 16-byte chunk of a row is clamped at each dword
    position (level 1 is 151-153 wide and adds w % 4 of 3, 0, 1 on the library's own pitch).  Packed rows: the byte path's
    per-pixel clamp at the same widths."""
    _check(ctx, oracle, _pair(w, 91, seed=11), 2, stride=w if packed else None)


@pytest.mark.parametrize("w,stride,offset", [
    (182, 183, 0),      # odd row stride: byte path
    (182, 192, 1),      # a view one byte into a wider buffer: byte path
    (184, 188, 0),      # stride w + 4, w % 4 == 0: dword loads allowed (16-byte staging where the band pitch allows)
    (184, 184, 0),      # contiguous: 16-byte staging
], ids=["stride_w+1", "offset_1", "stride_w+4", "contiguous"])
def test_level0_caller_layouts(ctx, oracle, w, stride, offset):
    _check(ctx, oracle, _pair(w, 96, seed=13), 2, stride, offset)


def _sparse(w=182, h=96):
    """test_texture_extremes' `sparse` pattern cut to w x h: flat 30 with a faint ramp and one bright rectangle.  On the oracle
    that pattern alone yields only corners of score 187-189 (at full size too), so that no cell falls back to minThFAST: a faint
    rectangle (contrast 16: corner scores 14-15) is added two cells to the right, and a faint patch below the bright
    rectangle, inside a cell that also holds one of its corners (weak maxima in the bucket of an iniThFAST cell)."""
    img = np.full((h, w), 30, np.uint8)
    img[30:60, 30:70] = 220
    img[30:60, 110:150] = 46
    img[66:76, 34:44] = 46
    return (img.astype(int) + (np.arange(w)[None, :] * 5 + np.arange(h)[:, None] * 3) % 7).astype(np.uint8)


def test_counts_from_counters(ctx, oracle):
    """Cells with a corner >= iniThFAST (count = cell_hi) next to cells that fall back to minThFAST (count = the bucket)."""
    frames = np.stack([_sparse(), _sparse()[::-1].copy()])
    for f in range(2):
        sc = _cand0(oracle, frames[f], 2)
        assert (sc < INI).any() and (sc >= INI).any(), f          # both kinds of cell are really present
    _check(ctx, oracle, frames, 2)


def test_score_ties(ctx, oracle):
    """5-px patterns of test_texture_extremes: equal scores everywhere, the rank inside a cell decides the order.  Frame 0 is
    that test's pattern (diagonal stripes: no level-0 corner at this size, 187 candidates on level 1), frame 1 the
    checkerboard proper (29 level-0 candidates of one score, 232 on level 1)."""
    y, x = np.indices((96, 182))
    a = ((x + y) // 5 % 2 * 200 + 20).astype(np.uint8)
    b = ((x // 5 + y // 5) % 2 * 200 + 20).astype(np.uint8)
    _check(ctx, oracle, np.stack([a, b]), 2)


def _corners_at(img, th):
    """FAST-9/16 segment test: True where 9 contiguous ring pixels are all brighter than v + th or all darker than v - th
    (such a pixel's score is >= th).  The 3-pixel image border is False."""
    ring = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
    a = img.astype(np.int32)
    h, w = a.shape
    v = a[3:h - 3, 3:w - 3]
    r = np.stack([a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in ring])
    out = np.zeros((h, w), bool)
    for m in (r > v + th, r < v - th):
        m2 = np.concatenate([m, m[:8]])
        out[3:h - 3, 3:w - 3] |= np.any([np.all(m2[k:k + 9], axis=0) for k in range(16)], axis=0)
    return out


@pytest.mark.parametrize("h", [96, 128])
def test_list_overflow(ctx, oracle, h):
    """Uniform noise: the scored-pixel list of a band overflows and the per-cell row scan runs.  Checked per band on the
    input: level 0 of a 182-wide frame has five 30-px cell columns from x = 16, the first four form one band (tile pitch 144),
    whose detection rectangle in the first cell row is x 19..138, y 19..(19 + cell height - 1); the band scores every pixel
    there that passes the segment test at minThFAST, and more than FC_NZ = 1024 of them overflow its list.
    The issue's sign -- more than 1024 level-0 candidates in total -- holds at 182 x 128 only (at 182 x 96 the oracle finds
    about 850: 9 % of the 150 x 64 detection pixels are local maxima) and is asserted there; both sizes are compared."""
    frames = np.random.default_rng(5).integers(0, 256, (2, h, 182), dtype=np.uint8)
    hcell = -(-(h - 32) // ((h - 32) // 30))                  # ceil(height / nRows) of the detection area
    for f in range(2):
        assert _corners_at(frames[f], MN)[19:19 + hcell, 19:139].sum() > 1024, f
        if h == 128:
            assert len(_cand0(oracle, frames[f], 2)) > 1024, f
    _check(ctx, oracle, frames, 2)
