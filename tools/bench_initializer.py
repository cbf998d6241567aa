#!/usr/bin/env python3
"""Times ccm_initialize (the monocular Initializer, src/Initializer.cpp) at N = 100, 300 and 1000 matches with 200 iterations on
general-depth scenes with a fifth of the matches wrong (tests/initializer_ref.make_two_view).

  wall     host clock around the call (it ends with a synchronisation), median [p10, p90] of --reps repetitions after --warmup
  device   HIP events on the context's stream around the same call: first upload to last download, the host work between the
           two launches (selection, decomposition) included
  kernels  with --kernel-stats N=FILE ...: the duration of k_init_hypotheses and k_init_check_rt at size N from the kernel statistics
           of a separate run `rocprofv3 --kernel-trace --stats -- python tools/bench_initializer.py --sizes N` (tracing slows the
           host, so the two runs are not mixed)

No baseline: the reference needs OpenCV to build, and the numpy restatement the tests use is not a fair one.
Output: profiles/<tag>_initializer.json and one summary line."""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (first, so that the library binds to the same HIP runtime as in the tests)

from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.initializer import make_draws  # noqa: E402
import initializer_ref as ref  # noqa: E402


def stats(ts_ms):
    t = np.asarray(ts_ms)
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def kernel_stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in ("k_init_hypotheses", "k_init_check_rt"):
                if k in row["Name"]:
                    out[k] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100, 300, 1000])
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--kernel-stats", nargs="*", default=[], metavar="N=FILE",
                    help="kernel statistics CSV of a run at size N under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    ctx = _lib.Context(0); lib = _lib.load(); p = _lib.ptr
    stream = torch.cuda.ExternalStream(ctx.stream)
    rng = np.random.default_rng(7)
    result = {"iterations": a.iterations, "sizes": {}}
    for n in a.sizes:
        pr = ref.make_two_view(rng, n, 0.2, "general")
        d = make_draws(rng, n, a.iterations)
        n1 = len(pr["kp1"])
        p3d = np.zeros((n1, 3), "f4"); tri = np.zeros(n1, "u1")
        K = pr["K"]
        pb = _lib.InitializerProblem(n1, p(pr["kp1"]), len(pr["kp2"]), p(pr["kp2"]), p(pr["matches12"]), float(K[0]), float(K[1]), float(K[2]),
                                     float(K[3]), 1.0, a.iterations, 1.0, 50, p(d))
        res = _lib.InitializerResult()
        res.p3d, res.triangulated = p(p3d), p(tri)
        wall, dev = [], []
        for r in range(a.warmup + a.reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            ctx.check(lib.ccm_initialize(ctx.handle, C.byref(pb), C.byref(res)))
            t1 = time.perf_counter()
            e1.record(stream); e1.synchronize()
            if r >= a.warmup:
                wall.append((t1 - t0) * 1e3); dev.append(e0.elapsed_time(e1))
        result["sizes"][str(n)] = {"initialized": int(res.initialized), "model": "HF"[res.model], "wall": stats(wall), "device": stats(dev)}
    for item in a.kernel_stats:
        n, path = item.split("=", 1)
        result["sizes"].setdefault(n, {})["kernels"] = kernel_stats(path)
    out = a.out or os.path.join(ROOT, "profiles", "%s_initializer.json" % a.tag)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    ctx.close()


if __name__ == "__main__":
    main()
