"""Frame::UndistortKeyPoints / Frame::ComputeImageBounds (src/Frame.cpp:277-337) restated in numpy float64, independent of the library
and of the oracle: cv::undistortPoints as Frame.cpp:295 calls it (R empty, P = mK) in its classic fixed-count form.  Every elementwise
numpy operation is one IEEE double operation, in the order include/ccm_hot.h states them.  Shared by tests/test_undistort_cpu.py and
tests/test_frame_undistort_gpu.py."""
import numpy as np

FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
# cslam/conf/vi_euroc.yaml (Camera.fx .. Camera.p2; no k3), the 752 x 480 camera
EUROC = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, k1=-0.28340811, k2=0.07395907, p1=0.00019359, p2=1.76187114e-05, k3=0.0)
# a synthetic camera: k3 != 0 and tangential terms of visible size; its denominator stays positive over 752 x 480
# (test_undistort_cpu.test_synthetic_camera_denominator_stays_positive)
SYNTH = dict(fx=420.0, fy=415.0, cx=380.5, cy=235.25, k1=-0.21, k2=0.09, p1=0.004, p2=-0.003, k3=-0.012)
# the early return: k1 == 0 with every other coefficient set
K1_ZERO = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, k1=0.0, k2=0.07395907, p1=0.004, p2=-0.003, k3=0.01)
WIDTH, HEIGHT = 752, 480
GRID_COLS, GRID_ROWS = 75, 48                       # FRAME_GRID_COLS, FRAME_GRID_ROWS (include/cslam/Frame.h:51-52)
# ComputeImageBounds of EUROC at 752 x 480: recorded results of this restatement (min_x, max_x, min_y, max_y)
EUROC_BOUNDS = (-135.79564, 895.5073, -92.875015, 565.5531)


def widened(cam):
    """The nine values rounded to float (mK, mDistCoef are CV_32F) and widened to double."""
    return {k: np.float64(np.float32(cam[k])) for k in FIELDS}


def denominator(cam, x, y):
    c = widened(cam)
    r2 = x * x + y * y
    return 1.0 + ((c["k3"] * r2 + c["k2"]) * r2 + c["k1"]) * r2


def undistort(cam, u, v, iters=5):
    """(u', v') float32 of the float32 points (u, v); iters = 5 is the definition."""
    c = widened(cam)
    u = np.asarray(u, np.float32); v = np.asarray(v, np.float32)
    if np.float32(cam["k1"]) == 0.0:                 # mvKeysUn = mvKeys (:279-283)
        return u.copy(), v.copy()
    ifx = 1.0 / c["fx"]; ify = 1.0 / c["fy"]
    x0 = (u.astype(np.float64) - c["cx"]) * ifx
    y0 = (v.astype(np.float64) - c["cy"]) * ify
    x = x0.copy(); y = y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((c["k3"] * r2 + c["k2"]) * r2 + c["k1"]) * r2)
        dx = ((2.0 * c["p1"]) * x) * y + c["p2"] * (r2 + (2.0 * x) * x)
        dy = c["p1"] * (r2 + (2.0 * y) * y) + ((2.0 * c["p2"]) * x) * y
        x = (x0 - dx) * icdist; y = (y0 - dy) * icdist
    return (c["fx"] * x + c["cx"]).astype(np.float32), (c["fy"] * y + c["cy"]).astype(np.float32)


def image_bounds(cam, width, height, grid_cols=GRID_COLS, grid_rows=GRID_ROWS):
    """(min_x, max_x, min_y, max_y, inv_w, inv_h) as float32 (:309-337, :87-88)."""
    if np.float32(cam["k1"]) != 0.0:
        x, y = undistort(cam, np.array([0, width, 0, width], np.float32), np.array([0, 0, height, height], np.float32))
        b = [min(x[0], x[2]), max(x[1], x[3]), min(y[0], y[1]), max(y[2], y[3])]
    else:
        b = [np.float32(0), np.float32(width), np.float32(0), np.float32(height)]
    inv_w = np.float32(grid_cols) / np.float32(b[1] - b[0])
    inv_h = np.float32(grid_rows) / np.float32(b[3] - b[2])
    return tuple(np.float32(t) for t in b) + (inv_w, inv_h)


def integer_grid(width=WIDTH, height=HEIGHT):
    """The (width + 1) x (height + 1) integer grid as float32 (u, v)."""
    gu, gv = np.meshgrid(np.arange(width + 1, dtype=np.float32), np.arange(height + 1, dtype=np.float32))
    return gu.ravel(), gv.ravel()
