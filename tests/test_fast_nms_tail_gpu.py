"""The tail of k_fast_cells' list NMS: a cell's local maxima collected in its bucket (tile column and row packed with the
score), ranked in row-major order and written to the cell's slots; buckets of exactly 0, 1, 63, 64 and 65 entries (the sizes
at which a ranking that holds a bucket in one wave's registers would change form: that variant was built against these
tests, measured and dropped), buckets above 64 in every band shape, the bucket overflow that sends a band to the row scan,
and the threshold choice inside a bucket.  The input is a dot lattice: a flat background of 100 with single pixels of value 100 + c at
(19 + 4a + 2b, 19 + 3b), clipped to the detection area.  No two dots lie on each other's FAST ring or in each other's 3x3
neighbourhood, so every dot is an isolated corner of score c - 1 and a cell's local maxima can be counted on the input.
All dots of a frame that share c share a score, so the order inside a cell is decided by the rank alone.  Every case extracts
a 2-frame batch -- frame 1 is frame 0 flipped top to bottom -- and compares, per frame, the FAST candidates of every level and
the keypoints and descriptors with the CPU oracle.  The counts a case is about are asserted on the oracle's candidates
before the GPU is used."""
import numpy as np
import pytest

from motioncheck_ccm_slam_amd.orb import ORBextractor

pytestmark = pytest.mark.gpu

NF, SF, NL, INI, MN = 300, 1.2, 2, 20, 7
STRONG, WEAK = 30, 12           # dot contrasts: scores 29 >= iniThFAST and 7 <= 11 < iniThFAST
FC_NZ = 1024                    # k_fast_cells' list of scored pixels
BAND_CELLS = 4                  # cells of a band, and the bucket capacities of 4-, 2- and 1-cell bands
CAP = {4: 119, 2: 239, 1: 479}


def _grid(w, h):
    """Level 0's cell grid as the extractor lays it out: columns, rows, cell width and height.  Cell (j, i) owns the
    maxima at x in [19 + j * wc, 19 + (j + 1) * wc), y in [19 + i * hc, 19 + (i + 1) * hc)."""
    nc, nr = (w - 32) // 30, (h - 32) // 30
    return nc, nr, -(-(w - 32) // nc), -(-(h - 32) // nr)


def _dots(w, h):
    """[(x, y, a, b)] of the lattice inside the detection area, row-major."""
    out = []
    for b in range((h - 38 + 2) // 3 + 1):
        y = 19 + 3 * b
        if y >= h - 19:
            break
        for a in range(-b, w):
            x = 19 + 4 * a + 2 * b
            if x < 19:
                continue
            if x >= w - 19:
                break
            out.append((x, y, a, b))
    return out


def _cell_of(x, y, w, h):
    nc, nr, wc, hc = _grid(w, h)
    return (x - 19) // wc, (y - 19) // hc


def _image(w, h, contrast=lambda x, y, a, b: STRONG):
    """The lattice; contrast(x, y, a, b) is the dot's c, 0 = no dot."""
    img = np.full((h, w), 100, np.uint8)
    for x, y, a, b in _dots(w, h):
        img[y, x] = 100 + contrast(x, y, a, b)
    return img


def _pair(img):
    return np.stack([img, img[::-1].copy()])


def _cells0(oracle, img):
    """Level 0 on the oracle: {(j, i): [scores of the cell's candidates]}."""
    h, w = img.shape
    r = oracle.orb_extract(oracle.default_params(NF, SF, NL, INI, MN), img, cand_level=0)
    nc, nr, wc, hc = _grid(w, h)
    cells = {(j, i): [] for j in range(nc) for i in range(nr)}
    for (x, y), s in zip(r["cand_xy"], r["cand_score"]):         # candidate positions count from the detection area's corner (16, 16)
        cells[((int(x) - 3) // wc, (int(y) - 3) // hc)].append(int(s))
    return cells


def _check(ctx, oracle, frames):
    """frames [2, h, w] on the device with rows on dword boundaries (level 0 is read in place, 16 bytes per lane)."""
    import torch
    n, h, w = frames.shape
    stride = (w + 3) & ~3
    plane = stride * h + 64
    host = np.random.default_rng(w * 1000 + h).integers(0, 256, plane * n + 4096, dtype=np.uint8)
    for f in range(n):
        np.lib.stride_tricks.as_strided(host[f * plane:], shape=(h, w), strides=(stride, 1))[...] = frames[f]
    buf = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    ex = ORBextractor(NF, SF, NL, INI, MN, ctx=ctx)
    ex.extract_dev(buf.data_ptr(), w, h, stride, plane, n)
    kps, desc, counts = ex.fetch()
    par = oracle.default_params(NF, SF, NL, INI, MN)
    for f in range(n):
        for l in range(NL):
            r = oracle.orb_extract(par, frames[f], cand_level=l)
            xy, sc = ex.fast_candidates(f, l)
            assert len(xy) == len(r["cand_xy"]) and (xy == r["cand_xy"]).all() and (sc == r["cand_score"]).all(), (f, l)
        c = int(counts[f])
        assert c == len(r["kps"]), f
        for name in kps.dtype.names:
            assert (kps[f, :c][name] == r["kps"][name]).all(), (f, name)
        assert (desc[f, :c] == r["desc"]).all(), f
    del buf


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_exact_bucket(ctx, oracle, n):
    """182 x 96: cell (1, 0), inside the 4-cell band of the first cell row, keeps its first n dots in row-major order: an
    empty bucket, a single entry, and a wave's 64 lanes one short, full and one over.  The other cells keep the full lattice."""
    w, h = 182, 96
    order = {}
    for x, y, a, b in _dots(w, h):
        if _cell_of(x, y, w, h) == (1, 0):
            order[(x, y)] = len(order)
    assert len(order) >= 65
    img = _image(w, h, lambda x, y, a, b: STRONG if order.get((x, y), -1) < n else 0)
    cells = _cells0(oracle, img)
    assert len(cells[(1, 0)]) == n
    assert all(len(v) > 64 for (j, i), v in cells.items() if j < BAND_CELLS and (j, i) != (1, 0))
    _check(ctx, oracle, _pair(img))


@pytest.mark.parametrize("w,h", [(182, 96), (96, 96)])
def test_buckets_above_64(ctx, oracle, w, h):
    """The full lattice: buckets of more than 64 local maxima and no more than the bucket's capacity -- 119 in the 4-cell
    bands and 479 in the 1-cell bands of 182 x 96, 239 in the 2-cell bands of 96 x 96: every band shape.
    The cells are 32 rows high: 11 lattice rows in the first cell row (82-83 maxima in a full-width cell, 88 at 96 x 96) and
    9 in the second (67-68, 72); the narrower last cell column holds 66 / 54 and 72 / 58.  So every cell of a 4-cell band is
    above 64, and both other band shapes have bands with such a cell."""
    img = _image(w, h)
    nc, nr = _grid(w, h)[:2]
    for f in _pair(img):
        cells = _cells0(oracle, f)
        strided = set()                                       # band shapes with a bucket above 64
        for i in range(nr):
            for j0 in range(0, nc, BAND_CELLS):
                band = [len(cells[(j, i)]) for j in range(j0, min(j0 + BAND_CELLS, nc))]
                assert max(band) <= CAP[len(band)], (j0, i, band)
                assert len(band) < BAND_CELLS or min(band) > 64, (j0, i, band)
                if max(band) > 64:
                    strided.add(len(band))
        assert strided == ({4, 1} if w == 182 else {2}), strided
    _check(ctx, oracle, _pair(img))


def test_bucket_overflow(ctx, oracle):
    """182 x 91, one cell row of 59 rows: cells of the 4-cell band hold more local maxima than a bucket (119) while the band's
    scored pixels -- the dots: nothing else passes the segment test -- stay below FC_NZ, so the row scan is entered through the
    bucket test and not through the list's."""
    w, h = 182, 91
    img = _image(w, h)
    for f in _pair(img):
        cells = _cells0(oracle, f)
        band = [len(cells[(j, 0)]) for j in range(BAND_CELLS)]
        assert max(band) > CAP[BAND_CELLS] and sum(band) < FC_NZ, band
    assert sum(1 for x, y, a, b in _dots(w, h) if _cell_of(x, y, w, h)[0] < BAND_CELLS) < FC_NZ
    _check(ctx, oracle, _pair(img))


@pytest.mark.parametrize("every_row", [True, False], ids=["buckets_above_64", "buckets_below_64"])
def test_both_thresholds(ctx, oracle, every_row):
    """182 x 96: strong and weak dots alternate in the even cell columns, the odd ones hold weak dots only.  Where a strong
    dot exists the cell's count is that of the strong ones and the weak ones are neither written nor counted in a rank;
    elsewhere the count is the whole bucket.  With every lattice row a full-width bucket holds 67-83 maxima, with every other
    row at most 64."""
    w, h = 182, 96

    def contrast(x, y, a, b):
        if not every_row and b % 2:
            return 0
        return STRONG if _cell_of(x, y, w, h)[0] % 2 == 0 and (a + b // (1 if every_row else 2)) % 2 == 0 else WEAK
    img = _image(w, h, contrast)
    dots = {}
    for x, y, a, b in _dots(w, h):
        if contrast(x, y, a, b):
            dots[_cell_of(x, y, w, h)] = dots.get(_cell_of(x, y, w, h), 0) + 1
    if every_row:                                             # (a bucket holds the cell's strong AND weak dots)
        assert all(v > 64 for (j, i), v in dots.items() if j < BAND_CELLS), dots
    else:
        assert all(0 < v <= 64 for v in dots.values()), dots
    for f in _pair(img):
        cells = _cells0(oracle, f)
        hi = [k for k, v in cells.items() if v and min(v) == STRONG - 1]
        lo = [k for k, v in cells.items() if v and max(v) == WEAK - 1]
        assert hi and lo and len(hi) + len(lo) == len(cells), (hi, lo)
    for k, v in _cells0(oracle, img).items():                 # (frame 0, whose cells are the lattice's)
        assert len(v) == dots[k] if v[0] == WEAK - 1 else 0 < len(v) < dots[k], (k, len(v), dots[k])
    _check(ctx, oracle, _pair(img))
