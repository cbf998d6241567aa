"""CPU-side checks of the frame-BoW entry points (ccm_frame_compute_bow, ccm_frame_search_by_bow, ccm_search_by_bow_frames): the
library exports them with the prototypes include/ccm_hot.h declares, the ABI version is unchanged, the ctypes mirror and the shim
call them with the declared argument counts.  No GPU work here; tests/test_frame_bow_gpu.py checks what they compute."""
import os
import re
import shutil
import subprocess

import pytest

from motioncheck_ccm_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ccm_frame_compute_bow", "ccm_frame_search_by_bow", "ccm_search_by_bow_frames")

# the prototypes of the issue, as function-pointer types: assigning the library's symbols to them compiles only if the header agrees
PROBE = r'''
#include "ccm_hot.h"
#include <stdio.h>
typedef int (*compute_bow_t)(ccm_ctx*, ccm_frame*, ccm_vocabulary*, int, int32_t*, double*, int32_t*);
typedef int (*search_by_bow_t)(ccm_ctx*, const ccm_frame*, ccm_frame*, const ccm_bow_options*, const uint8_t*, int, int32_t*);
typedef int (*search_by_bow_frames_t)(ccm_ctx*, const ccm_frame*, int, ccm_frame* const*, const ccm_bow_options*, const uint8_t*,
                                      const int32_t*, const uint8_t*, int32_t*, int32_t*);
int main(void) {
    compute_bow_t a = ccm_frame_compute_bow;
    search_by_bow_t b = ccm_frame_search_by_bow;
    search_by_bow_frames_t c = ccm_search_by_bow_frames;
    ccm_bow_options o = {0.7f, 1, 50, 0};
    /* null handles are refused before anything touches a device */
    printf("%d %d %d %d %d\n", ccm_abi_version(), CCM_ABI_VERSION, a(0, 0, 0, 4, 0, 0, 0), b(0, 0, 0, &o, 0, 15, 0), c(0, 0, 0, 0, &o, 0, 0, 0, 0, 0));
    return 0;
}
'''


def _header():
    txt = open(os.path.join(ROOT, "include", "ccm_hot.h")).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _n_args(text, name):
    m = re.search(r"\b%s\s*\(" % name, text)
    assert m, name
    depth, j = 0, m.end() - 1
    while True:
        depth += text[j] == "("; depth -= text[j] == ")"
        if depth == 0:
            break
        j += 1
    return len([a for a in text[m.end():j].split(",") if a.strip()])


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ccm_abi_version() == 3 == _lib.ABI_VERSION
    h = _header()
    for name, n in zip(NAMES, (7, 7, 10)):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert _n_args(h, name) == n == len(getattr(lib, name).argtypes), name


def test_prototypes_are_the_declared_ones(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "motioncheck_ccm_slam_amd")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", inc, str(src), "-o", str(exe), "-L", libdir,
                           "-lccm_hot", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["3", "3", "-1", "-1", "-1"], out.stdout + out.stderr


def test_python_mirror_and_shim_use_the_calls():
    from motioncheck_ccm_slam_amd.frame import DeviceFrame
    from motioncheck_ccm_slam_amd.matcher import ORBmatcher
    from motioncheck_ccm_slam_amd.tracking import Tracking
    assert callable(DeviceFrame.compute_bow) and callable(ORBmatcher.SearchByBoWHandle) and callable(ORBmatcher.SearchByBoWFrames)
    assert callable(Tracking.TrackReferenceKeyFrame)
    h = _header()
    shim = {f: re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "shim", f)).read(), flags=re.S))
            for f in ("cslam_tracking.cpp", "cslam_sim3solver.cpp")}
    for f, names in (("cslam_tracking.cpp", NAMES[:2]), ("cslam_sim3solver.cpp", NAMES[2:])):
        assert "Tracking::TrackReferenceKeyFrame" in shim["cslam_tracking.cpp"]
        for name in names:
            assert _n_args(shim[f], name) == _n_args(h, name), (f, name)
