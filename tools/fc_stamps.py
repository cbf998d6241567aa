#!/usr/bin/env python3
"""Where does a band of k_fast_cells spend its cycles?  (diagnostic build -DFC_STAMPS)

usage: tools/fc_stamps.py --build DIR [--src TREE]     copy TREE's csrc/ and include/ (default: this tree's) into DIR and build
                                                       DIR/libccm_hot_stamps.so there (EXTRA=-DFC_STAMPS; no GPU needed, the shipped
                                                       library is not touched).  TREE may be a checkout of another commit.
       tools/fc_stamps.py --lib DIR/libccm_hot_stamps.so
                                                       run 256-frame extractions of the bench frames on one lane in a fresh process
                                                       under a time limit, and print the phase medians over every band of the last one

The stamps are s_memtime of wave 0 (slots 0-7) and of the last wave (slots 8-15) at the phase boundaries the kernel marks with
FC_STAMP(): 0 start, 6 band record arrived, 5 everything scalar arrived (the pixel loads can be issued), 7 this wave's pixels
arrived and stored, 1 staged (barrier), 2 every pixel scored (barrier), 3 local maxima listed (barrier), 4 written.  The library is
loaded through CCM_HOT_LIB, as tools/ab_orb.sh loads alternative builds."""
import argparse
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT = 200          # seconds for the measuring process


def build(dst, src):
    pkg = os.path.join(dst, "pkg")
    for sub, rel in (("pkg/csrc", "motioncheck_ccm_slam_amd/csrc"), ("include", "include")):
        d = os.path.join(dst, sub)
        os.makedirs(d, exist_ok=True)
        for f in os.listdir(os.path.join(src, rel)):
            p = os.path.join(src, rel, f)
            if os.path.isfile(p) and not f.endswith(".o"):
                shutil.copy2(p, d)
    subprocess.check_call(["make", "-s", "-C", os.path.join(pkg, "csrc"), "-j8", "EXTRA=-DFC_STAMPS"])
    out = os.path.join(dst, "libccm_hot_stamps.so")
    shutil.move(os.path.join(pkg, "libccm_hot.so"), out)
    print(out)


def measure():
    """(the child process: CCM_HOT_LIB and CCM_ORB_LANE_FRAMES are set)"""
    sys.path.insert(0, ROOT)
    import ctypes as C
    import numpy as np
    import torch
    from motioncheck_ccm_slam_amd import _lib, synth
    from motioncheck_ccm_slam_amd.orb import ORBextractor
    ctx = _lib.Context(0)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    frames = torch.from_numpy(synth.frames(0, 256)).cuda()
    lib = _lib.load()
    if not hasattr(lib, "ccm_debug_fc_stamps"):
        sys.exit("%s was not built with EXTRA=-DFC_STAMPS" % os.environ["CCM_HOT_LIB"])
    for rep in range(3):                                   # the third run's stamps: warm caches, settled clocks
        ex.extract_dev(frames.data_ptr(), 752, 480, 752, 752 * 480, 256); ctx.sync()
    n = 1 << 17
    buf = np.zeros((n, 16), np.uint64)
    lib.ccm_debug_fc_stamps.argtypes = [C.c_void_p, C.c_int]
    assert lib.ccm_debug_fc_stamps(buf.ctypes.data, n) == 0
    ok = buf[:, 4] > 0                                     # bands that ended on the listed path
    b = buf[ok].astype(np.int64)
    med = lambda a, c, w=0: float(np.median(b[:, w + c] - b[:, w + a]))
    print("workgroups with stamps: %d" % int(ok.sum()))
    head = [("start -> band descriptor arrived", 0, 6), ("-> everything scalar arrived, pixel loads can be issued", 6, 5),
            ("-> this wave's pixels arrived and stored", 5, 7), ("-> rest of the set-up + barrier", 7, 1)]
    for w, who in ((0, "wave 0"), (8, "last wave")):
        print("%s, medians:" % who)
        for name, a, c in head:
            print("  %-58s %7.0f" % (name, med(a, c, w)))
        print("  %-58s %7.0f" % ("start -> staged (barrier 1)", med(0, 1, w)))
        print("  %-58s %7.0f" % ("staged -> every pixel scored (barrier 2)", med(1, 2, w)))
        print("  %-58s %7.0f" % ("scored -> local maxima listed", med(2, 3, w)))
        print("  %-58s %7.0f" % ("local maxima -> written (end)", med(3, 4, w)))
        print("  %-58s %7.0f" % ("start -> end", med(0, 4, w)))
    print("workgroup start (wave 0) -> last wave's end: median %.0f  mean %.0f" % (np.median(b[:, 12] - b[:, 0]), (b[:, 12] - b[:, 0]).mean()))
    ctx.close()


def run(lib_path):
    env = dict(os.environ, CCM_HOT_LIB=os.path.abspath(lib_path),
               CCM_ORB_LANE_FRAMES="0")                    # one lane = ONE 256-frame launch: a second lane's k_fast_cells would overwrite the first's stamps
    return subprocess.run([sys.executable, os.path.abspath(__file__), "--measure"], env=env, timeout=TIME_LIMIT).returncode


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--build", metavar="DIR")
    ap.add_argument("--src", metavar="TREE", default=ROOT)
    ap.add_argument("--lib")
    ap.add_argument("--measure", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.measure:
        return measure()
    if a.build:
        build(a.build, a.src)
    if a.lib:
        sys.exit(run(a.lib))
    if not a.build and not a.lib:
        ap.error("--build DIR or --lib PATH")


if __name__ == "__main__":
    main()
