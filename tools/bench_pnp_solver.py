#!/usr/bin/env python3
"""Times the batched PnPsolver on a relocalisation shape: 8 candidate keyframes x 200 correspondences x (300 + 5) hypotheses.

With the reference's default epsilon (0.4) SetRansacParameters caps a solver of 200 correspondences at 70 iterations; the bench sets
epsilon = 0.2 so that every solver evaluates maxIterations = 300 hypotheses plus a reserve of 5 (probability 0.99, minInliers 8,
minSet 4, th2 5.991).  Half of the candidates are true (30 % of their matches wrong), the others have unrelated matches only.

  create       ccm_pnp_solver_create alone: upload, k_pnp_hypotheses, download + synchronisation, the record scan, k_pnp_refine,
               download + synchronisation
  first_return create + iterate(5) per candidate in turn up to the first pose that comes back + destroy
  cpu_one_core the same hypotheses and refinements on one CPU core: ccm_pnp_compute_pose (the kernels' arithmetic through the host
               compiler) for every minimal set and every record's inlier set, plus a numpy CheckInliers of every pose

Host clock around the synchronised calls, median [p10, p90] of --reps repetitions after --warmup.  The per-kernel times come from a
kernel trace of this program: run it once under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
tools/bench_pnp_solver.py --no-cpu --out /dev/null`, then again with --kernel-stats DIR/.../*_kernel_stats.csv.
Output: profiles/pnp_solver.json and one summary line."""
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

try:
    import torch  # noqa: F401  (first, so that the library binds to the same HIP runtime as in the tests)
except ImportError:
    pass

from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.pnpsolver import PnPSolver, make_draws  # noqa: E402
import pnp_solver_ref as ref  # noqa: E402


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def kernel_stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in ("k_pnp_hypotheses", "k_pnp_refine"):
                if k in row["Name"]:
                    out[k] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--n", type=int, default=200, help="correspondences per candidate")
    ap.add_argument("--reserve", type=int, default=5)
    ap.add_argument("--epsilon", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *_kernel_stats.csv of a run of this program")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_solver.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(4)
    problems = [ref.make_problem(rng, a.n, 0.3 if k % 2 == 0 else 1.0) for k in range(a.candidates)]
    flat = ref.flatten(problems)
    draws = make_draws(rng, [a.n] * a.candidates, 300 + a.reserve, 4)
    ctx = _lib.Context(0); lib = _lib.load(); p = _lib.ptr
    pb = _lib.PnpRansacProblem(a.candidates, p(flat["first"]), p(flat["n1"]), p(flat["K"]), p(flat["P2D"]), p(flat["P3Dw"]), p(flat["sigma2"]),
                               p(flat["kp_index"]), 0.99, 8, 300, 4, a.epsilon, 5.991, a.reserve, p(draws), 0)
    inl = np.zeros(int(flat["n1"].max()), np.uint8); Tcw = np.zeros(16, "f4")
    found, no_more, nin = C.c_int32(), C.c_int32(), C.c_int32()

    def create():
        h = C.c_void_p()
        ctx.check(lib.ccm_pnp_solver_create(ctx.handle, C.byref(pb), C.byref(h)))
        return h

    def first_return():
        h = create()
        live = [True] * a.candidates; turn = 0; hit = None
        while any(live) and hit is None:
            for i in range(a.candidates):
                if not live[i]:
                    continue
                turn += 1
                rc = lib.ccm_pnp_solver_iterate(h, i, 5, C.byref(found), C.byref(no_more), p(inl), C.byref(nin), p(Tcw))
                if rc < 0 or no_more.value:
                    live[i] = False
                if rc == 0 and found.value:
                    hit = (i, turn, nin.value); break
        lib.ccm_pnp_solver_destroy(h)
        return hit

    t_create, t_first = [], []
    hit = None
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter(); h = create(); t1 = time.perf_counter()
        lib.ccm_pnp_solver_destroy(h)
        t2 = time.perf_counter(); hit = first_return(); t3 = time.perf_counter()
        if r >= a.warmup:
            t_create.append(t1 - t0); t_first.append(t3 - t2)

    # what one create evaluated: the minimal sets and the records' inlier sets
    s = PnPSolver(draws=draws, reserve=a.reserve, ctx=ctx, **flat)
    s.SetRansacParameters(0.99, 8, 300, 4, a.epsilon, 5.991)
    hyps = [s.hypotheses(k) for k in range(a.candidates)]
    refs = [s.refinements(k) for k in range(a.candidates)]
    s.close()
    n_hyp = int(sum(len(h["count"]) for h in hyps)); n_ref = int(sum(len(r["count"]) for r in refs))
    result = {"shape": {"candidates": a.candidates, "correspondences": a.n, "hypotheses": n_hyp, "refinements": n_ref, "epsilon": a.epsilon},
              "first_return": {"candidate": hit[0], "turn": hit[1], "inliers": hit[2]} if hit else None,
              "create": stats(t_create), "create_round_robin_first_return_destroy": stats(t_first)}
    if not a.no_cpu:
        t_cpu = []
        for r in range(3):
            t0 = time.perf_counter()
            for pr, h, rf in zip(problems, hyps, refs):
                me = ref.max_error(pr["sigma2"])
                sets = [list(x) for x in h["sample"]] + [np.flatnonzero(h["inlier"][hyp]) for hyp in rf["hyp"]]
                Rt = np.zeros((len(sets), 12))
                for i, idx in enumerate(sets):
                    R, t = PnPSolver.compute_pose(pr["P3Dw"][idx], pr["P2D"][idx], pr["K"])
                    Rt[i, :9] = R.ravel(); Rt[i, 9:] = t
                ref.check_inliers(Rt, pr["K"], pr["P3Dw"], pr["P2D"], me)
            t_cpu.append(time.perf_counter() - t0)
        result["cpu_one_core_same_hypotheses_and_refinements"] = stats(t_cpu)
    if a.kernel_stats:
        result["kernels"] = kernel_stats(a.kernel_stats)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))
    ctx.close()


if __name__ == "__main__":
    main()
