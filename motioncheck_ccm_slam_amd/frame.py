"""Device-resident frames (include/ccm_hot.h "frame handles"): one `Frame`'s undistorted keypoints, descriptors, feature grid and
map-point ids kept on the GPU for the frame's lifetime, so that the per-frame calls of Tracking (SearchByProjection twice, pose
optimisation twice, src/Tracking.cpp:571-597 and :905-920) upload only their per-call inputs.

Map points are ids into the caller's map-point table, -1 = none (`Frame::mvpMapPoints`)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .matcher import FRAME_GRID_COLS, FRAME_GRID_ROWS, FrameGridView


class Camera:
    """ccm_camera: mK and mDistCoef of a Frame as the float values the reference stores (k3 = 0 when the settings file has none,
    src/Tracking.cpp:53-58).  `undistort` is Frame::UndistortKeyPoints (ccm_undistort_points), `image_bounds`
    Frame::ComputeImageBounds with the grid element sizes (ccm_image_bounds); both run on the host."""

    FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")

    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
        vals = np.array([fx, fy, cx, cy, k1, k2, p1, p2, k3], "f4")            # the float rounding of the nine values
        for name, v in zip(self.FIELDS, vals):
            setattr(self, name, float(v))
        self.struct = _lib.CameraStruct(*[float(v) for v in vals])

    def undistort(self, x, y):
        """(x_un, y_un) float32 of the float32 points (x, y)."""
        x = np.ascontiguousarray(x, "f4").reshape(-1); y = np.ascontiguousarray(y, "f4").reshape(-1)
        if len(x) != len(y):
            raise ValueError("x and y differ in length")
        xo = np.empty(max(len(x), 1), "f4"); yo = np.empty(max(len(x), 1), "f4")
        rc = _lib.load().ccm_undistort_points(C.byref(self.struct), len(x), _lib.ptr(x), _lib.ptr(y), _lib.ptr(xo), _lib.ptr(yo))
        if rc:
            raise _lib.CcmError(rc, "ccm_undistort_points")
        return xo[:len(x)], yo[:len(x)]

    def image_bounds(self, width, height, grid_cols=FRAME_GRID_COLS, grid_rows=FRAME_GRID_ROWS):
        """The _lib.FrameBounds (min_x, max_x, min_y, max_y, inv_w, inv_h) of a width x height image."""
        b = _lib.FrameBounds()
        rc = _lib.load().ccm_image_bounds(C.byref(self.struct), int(width), int(height), int(grid_cols), int(grid_rows), C.byref(b))
        if rc:
            raise _lib.CcmError(rc, "ccm_image_bounds")
        return b


def _bounds_struct(bounds, min_x, max_x, min_y, max_y):
    """bounds as a _lib.FrameBounds: given, or made from the four limits the way from_extract always has."""
    if bounds is not None:
        return bounds
    inv_w = np.float32(FRAME_GRID_COLS) / np.float32(np.float32(max_x) - np.float32(min_x))
    inv_h = np.float32(FRAME_GRID_ROWS) / np.float32(np.float32(max_y) - np.float32(min_y))
    return _lib.FrameBounds(float(np.float32(min_x)), float(np.float32(max_x)), float(np.float32(min_y)), float(np.float32(max_y)),
                            float(inv_w), float(inv_h))


class DeviceFrame:
    """A ccm_frame handle.  Build with `DeviceFrame(view, angle, ctx=...)` from host arrays or `DeviceFrame.from_extract` from the
    last extraction of an `ORBextractor`; release with `close()` (before the context goes)."""

    def __init__(self, view: FrameGridView | None = None, angle=None, ctx: _lib.Context | None = None, _handle=None):
        self.ctx = ctx or _lib.default_context(0)
        self.lib = self.ctx.lib
        if _handle is None:
            if view is None:
                raise ValueError("DeviceFrame needs a FrameGridView (or use DeviceFrame.from_extract)")
            self._angle = None if angle is None else np.ascontiguousarray(angle, "f4")
            if self._angle is not None and len(self._angle) != len(view.kx):
                raise ValueError("angle must have one entry per feature")
            g = view.struct()
            h = C.c_void_p()
            self.ctx.check(self.lib.ccm_frame_create(self.ctx.handle, C.byref(g), _lib.ptr(self._angle), C.byref(h)))
            _handle = h.value
        self.handle = _handle
        self.n = self.lib.ccm_frame_size(C.c_void_p(self.handle))

    @classmethod
    def from_extract(cls, extractor, image: int = 0, kx_un=None, ky_un=None, n: int = -1, min_x=0.0, max_x=752.0, min_y=0.0, max_y=480.0,
                     ctx: _lib.Context | None = None, camera: Camera | None = None, bounds=None):
        """Frame of image `image` of the extractor's last extract (ccm_frame_from_extract): octave, angle and descriptors stay on the
        device; kx_un / ky_un are the undistorted coordinates (None: the extracted ones).  n = keypoint count (-1: read it).
        With `camera` (a Camera) and / or `bounds` (Camera.image_bounds) the keypoints are undistorted on the device as the handle
        is built (ccm_frame_from_extract_camera) and no coordinates are passed; bounds=None then takes min_x .. max_y."""
        ctx = ctx or extractor.ctx
        lib = ctx.lib
        if camera is not None or bounds is not None:
            if kx_un is not None or ky_un is not None:
                raise ValueError("coordinate arrays and a camera exclude each other")
            b = _bounds_struct(bounds, min_x, max_x, min_y, max_y)
            h = C.c_void_p()
            ctx.check(lib.ccm_frame_from_extract_camera(ctx.handle, int(image), int(n), None if camera is None else C.byref(camera.struct),
                                                        C.byref(b), FRAME_GRID_COLS, FRAME_GRID_ROWS, C.byref(h)))
            return cls(ctx=ctx, _handle=h.value)
        kx = None if kx_un is None else np.ascontiguousarray(kx_un, "f4")
        ky = None if ky_un is None else np.ascontiguousarray(ky_un, "f4")
        if (kx is None) != (ky is None):
            raise ValueError("give both undistorted coordinate arrays or neither")
        if kx is not None:
            if n < 0:
                n = len(kx)
            if len(kx) < n or len(ky) < n:
                raise ValueError("coordinate arrays shorter than n")
        inv_w = np.float32(FRAME_GRID_COLS) / np.float32(np.float32(max_x) - np.float32(min_x))
        inv_h = np.float32(FRAME_GRID_ROWS) / np.float32(np.float32(max_y) - np.float32(min_y))
        h = C.c_void_p()
        ctx.check(lib.ccm_frame_from_extract(ctx.handle, int(image), int(n), _lib.ptr(kx), _lib.ptr(ky), float(np.float32(min_x)),
                                             float(np.float32(min_y)), float(inv_w), float(inv_h), FRAME_GRID_COLS, FRAME_GRID_ROWS,
                                             C.byref(h)))
        return cls(ctx=ctx, _handle=h.value)

    @classmethod
    def batch_from_extract(cls, extractor, first: int, count: int, camera: Camera | None = None, bounds=None, min_x=0.0, max_x=752.0,
                           min_y=0.0, max_y=480.0, ctx: _lib.Context | None = None):
        """The handles of images first .. first + count - 1 of the extractor's last extract, made by one call and one launch
        (ccm_frames_from_extract_camera); camera=None keeps the extracted coordinates.  All or nothing."""
        ctx = ctx or extractor.ctx
        b = _bounds_struct(bounds, min_x, max_x, min_y, max_y)
        hs = (C.c_void_p * max(int(count), 1))()
        ctx.check(ctx.lib.ccm_frames_from_extract_camera(ctx.handle, int(first), int(count), None if camera is None else C.byref(camera.struct),
                                                         C.byref(b), FRAME_GRID_COLS, FRAME_GRID_ROWS, hs))
        return [cls(ctx=ctx, _handle=hs[k]) for k in range(int(count))]

    def keypoints(self):
        """(kx, ky) float32: the handle's coordinates, mvKeysUn[i].pt (ccm_frame_get_keypoints)."""
        kx = np.empty(max(self.n, 1), "f4"); ky = np.empty(max(self.n, 1), "f4")
        self.ctx.check(self.lib.ccm_frame_get_keypoints(C.c_void_p(self.handle), _lib.ptr(kx), _lib.ptr(ky)))
        return kx[:self.n], ky[:self.n]

    @property
    def map_points(self) -> np.ndarray:
        out = np.empty(max(self.n, 1), "i4")
        self.ctx.check(self.lib.ccm_frame_get_map_points(C.c_void_p(self.handle), _lib.ptr(out)))
        return out[:self.n]

    @map_points.setter
    def map_points(self, ids):
        """None = all -1 (fill(mvpMapPoints, nullptr)); else one id per feature."""
        a = None
        if ids is not None:
            a = np.ascontiguousarray(ids, "i4")
            if a.shape != (self.n,):
                raise ValueError("map_points needs %d ids" % self.n)
        self.ctx.check(self.lib.ccm_frame_set_map_points(C.c_void_p(self.handle), _lib.ptr(a)))

    def grid(self):
        """(cell_first [cols*rows+1], cell_items) of the device-built grid (ccm_frame_debug_grid)."""
        first = np.zeros(FRAME_GRID_COLS * FRAME_GRID_ROWS + 1, "i4")
        items = np.zeros(max(self.n, 1), "i4")
        self.ctx.check(self.lib.ccm_frame_debug_grid(C.c_void_p(self.handle), _lib.ptr(first), _lib.ptr(items)))
        return first, items[:first[-1]]

    # ---- the keyframe side (ccm_frame_set_bow / _camera / _pose): what LocalMapping reads of a keyframe
    def set_bow(self, node):
        """FeatureVector node per feature (-1 = none); None clears it."""
        a = None
        if node is not None:
            a = np.ascontiguousarray(node, "i4").reshape(-1)
            if len(a) != self.n:
                raise ValueError("set_bow needs %d nodes" % self.n)
            if self.n == 0:
                a = np.full(1, -1, "i4")                       # an empty array may have no address; None would clear the bow
        self.ctx.check(self.lib.ccm_frame_set_bow(C.c_void_p(self.handle), _lib.ptr(a)))

    def compute_bow(self, voc, levelsup: int = 4, outputs: bool = True):
        """Frame::ComputeBoW / KeyFrame::ComputeBoW on the handle (ccm_frame_compute_bow): the descent of `voc` (an ORBVocabulary)
        on the handle's own descriptors, then the node directory built on the device -- the state set_bow leaves with the same
        nodes.  Returns (word_id, weight, node) per feature, node -1 for a stopped word (what ccm_bow_vector takes for mBowVec), or
        None with outputs=False (nothing but two counters is read back)."""
        if not outputs:
            self.ctx.check(self.lib.ccm_frame_compute_bow(self.ctx.handle, C.c_void_p(self.handle), voc.handle, int(levelsup), None, None, None))
            return None
        m = max(self.n, 1)
        wid = np.zeros(m, "i4"); w = np.zeros(m, "f8"); node = np.zeros(m, "i4")
        self.ctx.check(self.lib.ccm_frame_compute_bow(self.ctx.handle, C.c_void_p(self.handle), voc.handle, int(levelsup), _lib.ptr(wid),
                                                      _lib.ptr(w), _lib.ptr(node)))
        return wid[:self.n], w[:self.n], node[:self.n]

    def set_camera(self, K, scale_factors, level_sigma2):
        """K = (fx, fy, cx, cy); mvScaleFactors and mvLevelSigma2, as many levels each."""
        K = np.ascontiguousarray(K, "f4").reshape(4)
        sf = np.ascontiguousarray(scale_factors, "f4").reshape(-1); s2 = np.ascontiguousarray(level_sigma2, "f4").reshape(-1)
        if len(sf) != len(s2):
            raise ValueError("scale_factors and level_sigma2 differ in length")
        self.ctx.check(self.lib.ccm_frame_set_camera(C.c_void_p(self.handle), *[float(x) for x in K], _lib.ptr(sf), _lib.ptr(s2), len(sf)))

    def set_pose(self, Tcw, Ow):
        """Tcw [3][4] = [Rcw | tcw], Ow [3] = GetCameraCenter()."""
        T = np.ascontiguousarray(Tcw, "f4").reshape(12); O = np.ascontiguousarray(Ow, "f4").reshape(3)
        self.ctx.check(self.lib.ccm_frame_set_pose(C.c_void_p(self.handle), _lib.ptr(T), _lib.ptr(O)))

    def pose(self):
        """(Tcw [3][4], Ow [3]) as the DEVICE copy of the handle holds them (ccm_frame_get_pose, a test tap: synchronises)."""
        T = np.zeros(12, "f4"); O = np.zeros(3, "f4")
        self.ctx.check(self.lib.ccm_frame_get_pose(C.c_void_p(self.handle), _lib.ptr(T), _lib.ptr(O)))
        return T.reshape(3, 4), O

    def bow(self):
        """(order, nodes, first) of the device-resident node directory (ccm_frame_debug_bow)."""
        order = np.zeros(max(self.n, 1), "i4"); nodes = np.zeros(max(self.n, 1), "i4"); first = np.zeros(self.n + 1, "i4")
        nn = self.ctx.check(self.lib.ccm_frame_debug_bow(C.c_void_p(self.handle), _lib.ptr(order), _lib.ptr(nodes), _lib.ptr(first)))
        return order[:first[nn]], nodes[:nn], first[:nn + 1]

    def close(self):
        if getattr(self, "handle", None):
            self.lib.ccm_frame_destroy(C.c_void_p(self.handle))
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
