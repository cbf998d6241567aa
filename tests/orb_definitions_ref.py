"""The ORB extractor's stages restated from their published definitions (SURVEY.md section 12 and
ORBextractor.cpp:68-124, 579-639, 933-1024, 1205-1304): numpy only, float64 or exact integers, the obvious
formulation and not the fast one.  Neither the CPU oracle nor the kernels are consulted, so a mistake
they share shows as a disagreement with this file.

The keyword arguments after the `*` exist for tests/test_orb_definitions_cpu.py alone: each turns the
definition into one plausible mistake (arc of 8, `>=` in the NMS, ...) that the test inputs must expose.
"""
import math

import numpy as np

from motioncheck_ccm_slam_amd.pattern import PATTERN

EDGE = 19               # EDGE_THRESHOLD, ORBextractor.cpp:65
BORDER = EDGE - 3       # minBorderX = minBorderY, :941
HALF_PATCH = 15
CELL = 30               # W, :937

# Bresenham circle of radius 3, in ring order; only contiguity matters, not where it starts
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


# ---------------------------------------------------------------- FAST 9/16, score, 3x3 NMS
def fast_score_map(img, *, arc=9, strict_pixel=True):
    """For every interior pixel (3 px margin) the largest t' for which `arc` contiguous ring pixels are all
    < v - t' or all > v + t': the max over the 16 arcs and both signs of the min of the differences, minus 1.
    Returns an int array of the interior's shape (h-6, w-6); it is negative where no threshold >= 0 works."""
    img = np.asarray(img).astype(np.int64)
    h, w = img.shape
    v = img[3:h - 3, 3:w - 3]
    d = np.stack([v - img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])     # > 0: ring pixel darker than v
    best = np.full(v.shape, -256, np.int64)
    for sign in (1, -1):
        for k in range(16):
            arc_min = np.min(np.stack([sign * d[(k + i) % 16] for i in range(arc)]), axis=0)
            best = np.maximum(best, arc_min)
    return best - (1 if strict_pixel else 0)        # x < v - t'  <=>  v - x - 1 >= t'   (x <= v - t' for the mistake)


def fast(img, t, *, arc=9, strict_pixel=True, strict_nms=True):
    """FAST(img, t, nonmaxSuppression=true): (xy [n,2] as (x, y), score [n]) in row-major order."""
    img = np.asarray(img)
    h, w = img.shape
    if h < 7 or w < 7:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    s = fast_score_map(img, arc=arc, strict_pixel=strict_pixel)
    corner = s >= t
    score = np.zeros((h + 2, w + 2), np.int64)                 # non-corners, the margin and beyond hold 0
    score[4:h - 2, 4:w - 2] = np.where(corner, s, 0)
    keep = np.zeros((h, w), bool)
    keep[3:h - 3, 3:w - 3] = corner
    centre = score[1:h + 1, 1:w + 1]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                nb = score[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
                keep &= (centre > nb) if strict_nms else (centre >= nb)
    ys, xs = np.nonzero(keep)                                   # np.nonzero walks row-major
    return np.stack([xs, ys], axis=1).astype(np.int64), centre[ys, xs]


# ---------------------------------------------------------------- the per-cell loop, ORBextractor.cpp:937-998
def cell_candidates(level_img, ini_th, min_th, **fast_kw):
    """vToDistributeKeys of one level: (xy [n,2], score [n], skipped_cols, skipped_rows).  Coordinates are relative
    to the 16 px border (the reference adds minBorder back after the quadtree, :1012-1013).  skipped_* count the cell
    columns and rows that the two `continue` rules (:962, :971) leave out."""
    img = np.asarray(level_img)
    rows, cols = img.shape
    min_bx = min_by = BORDER
    max_bx, max_by = cols - EDGE + 3, rows - EDGE + 3
    width, height = float(max_bx - min_bx), float(max_by - min_by)
    n_cols, n_rows = int(width / CELL), int(height / CELL)
    w_cell, h_cell = math.ceil(width / n_cols), math.ceil(height / n_rows)
    xy, sc = [], []
    skipped_rows, skipped_cols = 0, set()
    for i in range(n_rows):
        ini_y = min_by + i * h_cell
        max_y = ini_y + h_cell + 6
        if ini_y >= max_by - 3:
            skipped_rows += 1
            continue
        max_y = min(max_y, max_by)
        for j in range(n_cols):
            ini_x = min_bx + j * w_cell
            max_x = ini_x + w_cell + 6
            if ini_x >= max_bx - 6:
                skipped_cols.add(j)
                continue
            max_x = min(max_x, max_bx)
            cell = img[ini_y:max_y, ini_x:max_x]
            kxy, ksc = fast(cell, ini_th, **fast_kw)
            if len(kxy) == 0:
                kxy, ksc = fast(cell, min_th, **fast_kw)
            xy.append(kxy + [j * w_cell, i * h_cell])
            sc.append(ksc)
    xy = np.concatenate(xy) if xy else np.zeros((0, 2), np.int64)
    sc = np.concatenate(sc) if sc else np.zeros(0, np.int64)
    return xy, sc, len(skipped_cols), skipped_rows


# ---------------------------------------------------------------- pyramid
def scale_factors(scale_factor, nlevels):
    """mvScaleFactor, float32 as the reference keeps it (:584-592)."""
    s = [np.float32(1.0)]
    for _ in range(1, nlevels):
        s.append(np.float32(s[-1] * np.float32(scale_factor)))
    return np.array(s, np.float32)


def level_sizes(w, h, scale_factor, nlevels):
    """Size(cvRound((float)cols*scale), cvRound((float)rows*scale)) with scale = 1.0f/mvScaleFactor[level] (:598, :1284-1285)."""
    inv = np.float32(1.0) / scale_factors(scale_factor, nlevels)
    lw = [int(np.rint(np.float32(np.float32(w) * i))) for i in inv]
    lh = [int(np.rint(np.float32(np.float32(h) * i))) for i in inv]
    return lw, lh


def resize(src, dw, dh, *, half_pixel=True):
    """Bilinear resize in float64, not rounded: destination x samples the source at (x+0.5)*sw/dw - 0.5, clamped to the image."""
    src = np.asarray(src, np.float64)
    sh, sw = src.shape
    o = 0.5 if half_pixel else 0.0
    fx = np.clip((np.arange(dw) + o) * sw / dw - o, 0, sw - 1)
    fy = np.clip((np.arange(dh) + o) * sh / dh - o, 0, sh - 1)
    x0 = np.floor(fx).astype(int); x1 = np.minimum(x0 + 1, sw - 1); ax = fx - x0
    y0 = np.floor(fy).astype(int); y1 = np.minimum(y0 + 1, sh - 1); ay = fy - y0
    top = src[y0][:, x0] * (1 - ax) + src[y0][:, x1] * ax
    bot = src[y1][:, x0] * (1 - ax) + src[y1][:, x1] * ax
    return top * (1 - ay)[:, None] + bot * ay[:, None]


# ---------------------------------------------------------------- 7x7 sigma = 2 blur, 8-bit fixed point
def blur_taps():
    g = np.exp(-np.arange(-3, 4) ** 2 / (2.0 * 2.0 ** 2))
    return np.rint(256 * g / g.sum()).astype(np.int64)


def blur(img):
    q = blur_taps()
    img = np.asarray(img).astype(np.int64)
    h, w = img.shape
    p = np.pad(img, ((0, 0), (3, 3)), mode="reflect")          # numpy's "reflect" is BORDER_REFLECT_101: the edge pixel is not repeated
    hor = sum(q[i] * p[:, i:i + w] for i in range(7))
    p = np.pad(hor, ((3, 3), (0, 0)), mode="reflect")
    ver = sum(q[i] * p[i:i + h, :] for i in range(7))
    return np.clip((ver + 32768) >> 16, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- IC_Angle, ORBextractor.cpp:68-95 and :621-638
def umax_table():
    """Half-widths of the radius-15 disc's rows, by the constructor's rule."""
    umax = [0] * (HALF_PATCH + 1)
    vmax = math.floor(HALF_PATCH * math.sqrt(2.0) / 2 + 1)
    vmin = math.ceil(HALF_PATCH * math.sqrt(2.0) / 2)
    for v in range(vmax + 1):
        umax[v] = int(np.rint(math.sqrt(HALF_PATCH * HALF_PATCH - v * v)))
    v0 = 0
    for v in range(HALF_PATCH, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


def ic_angle(level_img, x, y, *, umax=None):
    """Orientation by intensity centroid, degrees in [0, 360): atan2(m01, m10) over the disc around (x, y)."""
    img = np.asarray(level_img).astype(np.int64)
    umax = umax_table() if umax is None else umax
    m01 = m10 = 0
    for v in range(-HALF_PATCH, HALF_PATCH + 1):
        d = umax[abs(v)]
        u = np.arange(-d, d + 1)
        row = img[y + v, x - d:x + d + 1]
        m10 += int((u * row).sum())
        m01 += v * int(row.sum())
    return math.degrees(math.atan2(m01, m10)) % 360.0


# fastAtan2's published polynomial: atan(c) ~ c*(p1 + p3 c^2 + p5 c^4 + p7 c^6) for c in [0, 1]
ATAN2_P = (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128)


def fast_atan2_polynomial_error(n=2_000_001):
    """Worst error in degrees of the four-term polynomial against atan on a dense float64 grid of c in [0, 1]."""
    c = np.linspace(0.0, 1.0, n)
    c2 = c * c
    p1, p3, p5, p7 = ATAN2_P
    poly = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    return float(np.abs(np.degrees(poly - np.arctan(c))).max())


def angle_bound():
    """What an IC_Angle through fastAtan2 may differ from float64 atan2 by: the polynomial's own error plus 1e-3 degrees
    for evaluating it and the quadrant folding (90-a, 180-a, 360-a at up to 360) in float32."""
    return fast_atan2_polynomial_error() + 1e-3


def angle_diff(a, b):
    return np.abs((np.asarray(a, np.float64) - b + 180.0) % 360.0 - 180.0)


# ---------------------------------------------------------------- rotated BRIEF, ORBextractor.cpp:100-124
def sincos_deg(angle_deg):
    """float64 sin and cos of an angle in degrees.  The only rational sines of a whole number of degrees are 0, +-1/2 and +-1
    (Niven), all at multiples of 30; there the value is returned exactly, so that the exact ties of x/2 stay ties
    and are not turned into near-ties by the rounding of pi/180."""
    a = float(angle_deg)
    s, c = math.sin(math.radians(a)), math.cos(math.radians(a))
    if a % 30.0 == 0.0:
        s = round(2 * s) / 2 if abs(2 * s - round(2 * s)) < 1e-9 else s
        c = round(2 * c) / 2 if abs(2 * c - round(2 * c)) < 1e-9 else c
    return s, c


def brief_coords(angle_deg):
    """[256, 4] float64 sample offsets before rounding: (row, col) of the bit's first point, (row, col) of its second."""
    s, c = sincos_deg(angle_deg)
    p = PATTERN.reshape(256, 2, 2).astype(np.float64)           # [bit, point, (x, y)]
    px, py = p[..., 0], p[..., 1]
    return np.stack([px * s + py * c, px * c - py * s], axis=-1).reshape(256, 4)


def brief(blurred, x, y, angle_deg, *, half_up=False):
    """(bits [256] uint8, ambiguous [256] bool): bit k = I(first point) < I(second point) on the blurred level, offsets rounded
    to nearest with ties to even.  A bit is ambiguous when any of its four coordinates lies within 1e-4 of a half-integer:
    an evaluation in float32 may legitimately round those the other way."""
    f = brief_coords(angle_deg)
    r = (np.floor(f + 0.5) if half_up else np.rint(f)).astype(int)
    img = np.asarray(blurred)
    v0 = img[y + r[:, 0], x + r[:, 1]].astype(int)
    v1 = img[y + r[:, 2], x + r[:, 3]].astype(int)
    ambiguous = (np.abs(f - np.floor(f) - 0.5) < 1e-4).any(axis=1)
    return (v0 < v1).astype(np.uint8), ambiguous
