"""The frame-handle entry points (include/ccm_hot.h "frame handles") on the CPU: declared, exported, and refusing NULL contexts or
outputs with CCM_E_ARG before they touch a device.  No GPU work here."""
import ctypes as C
import os
import re

import numpy as np

from motioncheck_ccm_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_API = ["ccm_frame_create", "ccm_frame_from_extract", "ccm_frame_destroy", "ccm_frame_size", "ccm_frame_set_map_points",
             "ccm_frame_get_map_points", "ccm_frame_debug_grid", "ccm_frame_search_by_projection", "ccm_frame_search_by_projection_frame",
             "ccm_frame_pose_optimize"]
E_ARG = -1


def _header():
    txt = open(os.path.join(ROOT, "include", "ccm_hot.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_frame_entry_points_declared_and_exported():
    h = _header()
    assert re.search(r"typedef\s+struct\s+ccm_frame\s+ccm_frame\s*;", h)
    lib = _lib.load()
    for name in FRAME_API:
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert re.fullmatch(r"ccm_[a-z0-9_]+", name)
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert lib.ccm_abi_version() == 3 == _lib.ABI_VERSION         # additions only


def test_null_context_or_output_is_an_argument_error():
    lib = _lib.load()
    n = 4
    kx = np.zeros(n, "f4"); oc = np.zeros(n, "i4"); d = np.zeros((n, 32), np.uint8)
    p = _lib.ptr
    g = _lib.FrameGrid(n, p(kx), p(kx), p(oc), p(d), 0.0, 0.0, 0.1, 0.1, 75, 48)
    out = C.c_void_p(123)
    assert lib.ccm_frame_create(None, C.byref(g), None, C.byref(out)) == E_ARG
    assert out.value is None                                      # the output is cleared on failure
    assert lib.ccm_frame_from_extract(None, 0, -1, None, None, 0.0, 0.0, 0.1, 0.1, 75, 48, C.byref(out)) == E_ARG
    assert lib.ccm_frame_size(None) == E_ARG
    assert lib.ccm_frame_set_map_points(None, None) == E_ARG
    ids = np.zeros(n, "i4")
    assert lib.ccm_frame_get_map_points(None, p(ids)) == E_ARG
    first = np.zeros(75 * 48 + 1, "i4")
    assert lib.ccm_frame_debug_grid(None, p(first), p(ids)) == E_ARG
    m = np.zeros(n, "i4"); occ = np.zeros(n, np.uint8)
    assert lib.ccm_frame_search_by_projection(None, None, None, 0, *([None] * 9), 1.0, 0.8, p(m)) == E_ARG
    assert lib.ccm_frame_search_by_projection_frame(None, None, None, None, 0, *([None] * 8), p(occ), 7.0, 1, 100, p(m)) == E_ARG
    pose = np.zeros(7); intr = np.ones(4); outl = np.zeros(n, np.uint8); ni = np.zeros(1, "i4")
    assert lib.ccm_frame_pose_optimize(None, None, 0, None, None, 0, p(intr), p(pose), p(outl), p(ni)) == E_ARG
    lib.ccm_frame_destroy(None)                                   # harmless


def test_python_mirror_is_exposed():
    from motioncheck_ccm_slam_amd.frame import DeviceFrame
    from motioncheck_ccm_slam_amd.matcher import ORBmatcher
    from motioncheck_ccm_slam_amd.optimizer import Optimizer
    for name in ("from_extract", "map_points", "close", "grid"):
        assert hasattr(DeviceFrame, name), name
    assert callable(ORBmatcher.SearchByProjectionHandle) and callable(ORBmatcher.SearchByProjectionFrameHandle)
    assert callable(Optimizer.PoseOptimizationFrame)
