#!/usr/bin/env python3
"""Where does the level-0 quadtree workgroup of one frame spend its cycles?  (k_octree, diagnostic build -DOCT_STAMPS)

usage: tools/oct_stamps.py --build DIR                 copy csrc/ and include/ into DIR and build DIR/libccm_hot_stamps.so there
                                                       (EXTRA=-DOCT_STAMPS; no GPU needed, the shipped library is not touched)
       tools/oct_stamps.py --lib DIR/libccm_hot_stamps.so [--layout loop]
                                                       run one 256-frame extraction of the bench frames on the GPU and print the
                                                       phase table of the (frame 0, level 0) workgroup from ccm_debug_oct_stamps

The stamps are s_memtime of thread 0 at the phase boundaries the kernel marks with OCT_STAMP().  --layout chain (default) names the
stamps of the one-trip gather; --layout loop those of a tree from before it (a stamp per gather round, roots in passes of their
own), for a before / after table.  The library is loaded through CCM_HOT_LIB, as tools/ab_orb.sh loads alternative builds."""
import argparse
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(dst):
    pkg = os.path.join(dst, "pkg")
    for sub, src in (("pkg/csrc", "motioncheck_ccm_slam_amd/csrc"), ("include", "include")):
        d = os.path.join(dst, sub)
        os.makedirs(d, exist_ok=True)
        for f in os.listdir(os.path.join(ROOT, src)):
            p = os.path.join(ROOT, src, f)
            if os.path.isfile(p) and not f.endswith(".o"):
                shutil.copy2(p, d)
    subprocess.check_call(["make", "-s", "-C", os.path.join(pkg, "csrc"), "-j8", "EXTRA=-DOCT_STAMPS"])
    out = os.path.join(dst, "libccm_hot_stamps.so")
    shutil.move(os.path.join(pkg, "libccm_hot.so"), out)
    print(out)


def run(lib_path, layout):
    os.environ["CCM_HOT_LIB"] = os.path.abspath(lib_path)
    os.environ["CCM_ORB_LANE_FRAMES"] = "0"                # one lane = ONE 256-frame launch: every chunk's first workgroup would stamp, from CUs with clocks of their own
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
    if not hasattr(lib, "ccm_debug_oct_stamps"):
        sys.exit("%s was not built with EXTRA=-DOCT_STAMPS" % lib_path)
    lib.ccm_debug_oct_stamps.argtypes = [C.c_void_p, C.c_void_p]
    buf = np.zeros(64, np.uint64); n = np.zeros(1, np.int32)
    for rep in range(3):                                   # the third run's stamps: warm caches, settled clocks
        ex.extract_dev(frames.data_ptr(), 752, 480, 752, 752 * 480, 256); ctx.sync()
        assert lib.ccm_debug_oct_stamps(buf.ctypes.data, n.ctypes.data) == 0
    k = int(n[0]); t = buf[:k].astype(np.int64); d = np.diff(t)
    print("stamps: %d  total %d ticks   (level 0 of bench frame 0)" % (k, t[-1] - t[0]))
    print("raw deltas:", " ".join(str(int(v)) for v in d))
    if layout == "chain":
        head = ["counts loaded and scanned, offsets written", "barrier (offsets visible)", "cell search, keys fetched, roots counted, barrier",
                "roots numbered and written, barrier"]
    else:
        # start, a stamp per gather round, wave 0 stored, barrier, roots, 3 per pass, end (level 0 of the bench frames: 2 rounds)
        rounds = next(r for r in (1, 2, 3, 4) if (k - 5 - r) % 3 == 0)
        head = ["gather round %d: counts and slot offsets known" % r + (" (behind the keys of round %d)" % (r - 1) if r else "") for r in range(rounds)]
        head += ["wave 0's keys stored", "barrier (keys visible)", "roots: two passes over the keys, serial list"]
    rows = [(name, int(d[i])) for i, name in enumerate(head)]
    i, p = len(head), 0
    while i + 3 <= len(d) - 1:
        rows += [("pass %d: quadrants counted" % p, int(d[i])), ("pass %d: order chosen%s" % (p, " (careful: ranking)" if d[i + 1] > 2000 else ""), int(d[i + 1])),
                 ("pass %d: new list built, keys moved" % p, int(d[i + 2]))]
        i += 3; p += 1
    rows.append(("final selection", int(d[-1])))
    assert sum(c for _, c in rows) == t[-1] - t[0], "stamp layout does not match the library (try --layout %s)" % ("loop" if layout == "chain" else "chain")
    for name, c in rows:
        print("  %-66s %7d" % (name, c))
    gather = sum(c for _, c in rows[:len(head) - 1])
    print("  gather %d, roots %d, passes %d, final %d" % (gather, rows[len(head) - 1][1], sum(c for _, c in rows[len(head):-1]), rows[-1][1]))
    ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--build", metavar="DIR")
    ap.add_argument("--lib")
    ap.add_argument("--layout", choices=["chain", "loop"], default="chain")
    a = ap.parse_args()
    if a.build:
        build(a.build)
    if a.lib:
        run(a.lib, a.layout)
    if not a.build and not a.lib:
        ap.error("--build DIR or --lib PATH")


if __name__ == "__main__":
    main()
