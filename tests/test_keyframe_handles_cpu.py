"""The keyframe-handle entry points on the CPU: declared, exported, refusing NULL with CCM_E_ARG before they touch a device; the
Python mirror; and the node-directory builder (csrc/bow_directory.h) in a stand-alone program built with AddressSanitizer and UBSan,
run as a child process, against the numpy restatement.  No GPU work here."""
import os
import re
import subprocess

import numpy as np

from motioncheck_ccm_slam_amd import _lib
from keyframe_handles_ref import bow_cases, directory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_API = ["ccm_frame_set_bow", "ccm_frame_set_camera", "ccm_frame_set_pose", "ccm_frame_debug_bow", "ccm_create_new_map_points_frames",
           "ccm_fuse_select_batch_frames"]
E_ARG = -1


def test_new_entry_points_declared_and_exported():
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccm_hot.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_API:
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"\}\s*ccm_new_points_frames\s*;", h)
    assert lib.ccm_abi_version() == 3 == _lib.ABI_VERSION         # additions only


def test_null_is_an_argument_error():
    lib = _lib.load()
    p = _lib.ptr
    node = np.zeros(4, "i4"); tab = np.ones(8, "f4"); T = np.zeros(12, "f4"); O = np.zeros(3, "f4")
    assert lib.ccm_frame_set_bow(None, p(node)) == E_ARG
    assert lib.ccm_frame_set_camera(None, 1.0, 1.0, 0.0, 0.0, p(tab), p(tab), 8) == E_ARG
    assert lib.ccm_frame_set_pose(None, p(T), p(O)) == E_ARG
    assert lib.ccm_frame_debug_bow(None, p(node), p(node), p(node)) == E_ARG
    res = _lib.NewPointsResult(77, None, None, None, None, None, None)
    pb = _lib.NewPointsFrames(None, 0, None, None, None, None)
    assert lib.ccm_create_new_map_points_frames(None, pb, res) == E_ARG
    assert lib.ccm_create_new_map_points_frames(None, None, res) == E_ARG
    assert res.n_new == 77
    first = np.zeros(2, "i4")
    assert lib.ccm_fuse_select_batch_frames(None, 1, None, None, None, p(first), *([None] * 5), 3.0, 1, 50, None, None) == E_ARG


def test_python_mirror_is_exposed():
    from motioncheck_ccm_slam_amd.frame import DeviceFrame
    from motioncheck_ccm_slam_amd.mapping import LocalMapping
    from motioncheck_ccm_slam_amd.matcher import ORBmatcher
    for name in ("set_bow", "set_camera", "set_pose", "bow"):
        assert callable(getattr(DeviceFrame, name)), name
    assert callable(LocalMapping.CreateNewMapPointsFrames) and callable(ORBmatcher.FuseSelectBatchFrames)
    assert [f[0] for f in _lib.NewPointsFrames._fields_] == ["current", "n_kf", "neighbours", "F12", "epipole", "median_depth"]


def test_directory_builder_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bow_directory_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "support", "bow_directory_check.cpp"), "-o", exe])
    for j, node in enumerate(bow_cases() + [np.zeros(0, "i4")]):
        path = tmp_path / ("case%d.txt" % j)
        path.write_text("%d\n%s\n" % (len(node), " ".join(str(int(v)) for v in node)))
        out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
        for line, want in zip(out[:3], directory(node)):
            assert [int(v) for v in line.split()] == want.tolist()
