#!/usr/bin/env python3
"""Times the batched Sim3Solver on the loop closer's shape: 8 candidate keyframes x 100 correspondences x 300 hypotheses
(conf/config.yaml:122-128: probability 0.99, MinInliers 6, MaxIterations 300, 5 iterations per turn).

  create       ccm_sim3_solver_create alone: upload, the one launch, download, synchronisation
  first_return create + the round-robin of src/LoopFinder.cpp:288-346 (iterate(5) per candidate in turn) up to the first Sim3
               that comes back + destroy
  numpy_f64    context only: the float64 numpy restatement the tests compare against (tests/sim3_solver_ref.py), all
               hypotheses of the same inputs.  It is numpy, not the reference's C++.

Host clock around the synchronised calls (create synchronises before it returns), median [p10, p90] of --reps repetitions after
--warmup.  For the kernel alone run it once under `rocprofv3 --kernel-trace --stats -- python tools/bench_sim3_solver.py` and read
k_sim3_ransac from the kernel statistics.  Output: profiles/sim3_solver_bench.json and one summary line."""
import argparse
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
from motioncheck_ccm_slam_amd.sim3solver import make_draws  # noqa: E402
import sim3_solver_ref as ref  # noqa: E402


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--n", type=int, default=100, help="correspondences per candidate")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_solver_bench.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(4)
    # two true candidates (a fifth of the matches wrong), the others wrong ones, as in the chain test
    problems = [ref.make_solver_problem(rng, a.n, 0.2 if k in (2, 5) else 1.0, False) for k in range(a.candidates)]
    flat = ref.flatten(problems)
    draws = make_draws(rng, [a.n] * a.candidates, 300)
    ctx = _lib.Context(0); lib = _lib.load(); p = _lib.ptr
    pb = _lib.Sim3RansacProblem(a.candidates, p(flat["first"]), p(flat["n1"]), p(flat["fix_scale"]), p(flat["K1"]), p(flat["K2"]), p(flat["X1"]),
                                p(flat["X2"]), p(flat["max_err1"]), p(flat["max_err2"]), p(flat["indices1"]), 0.99, 6, 300, p(draws), None)
    inl = np.zeros(int(flat["n1"].max()), np.uint8); T12 = np.zeros(16, "f4")
    found, no_more, nin = C.c_int32(), C.c_int32(), C.c_int32()

    def create():
        h = C.c_void_p()
        ctx.check(lib.ccm_sim3_solver_create(ctx.handle, C.byref(pb), C.byref(h)))
        return h

    def first_return():
        h = create()
        live = [True] * a.candidates; turn = 0; hit = None
        while any(live) and hit is None:
            for i in range(a.candidates):
                if not live[i]:
                    continue
                turn += 1
                lib.ccm_sim3_solver_iterate(h, i, 5, C.byref(found), C.byref(no_more), p(inl), C.byref(nin), p(T12))
                if no_more.value:
                    live[i] = False
                if found.value:
                    hit = (i, turn, nin.value); break
        lib.ccm_sim3_solver_destroy(h)
        return hit

    t_create, t_first = [], []
    hit = None
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter(); h = create(); t1 = time.perf_counter()
        lib.ccm_sim3_solver_destroy(h)
        t2 = time.perf_counter(); hit = first_return(); t3 = time.perf_counter()
        if r >= a.warmup:
            t_create.append(t1 - t0); t_first.append(t3 - t2)
    h = create()
    n_hyp = [lib.ccm_sim3_solver_hypotheses(h, k, None, None, None, None) for k in range(a.candidates)]
    samples = []
    for k in range(a.candidates):
        s = np.zeros((n_hyp[k], 3), "i4"); lib.ccm_sim3_solver_hypotheses(h, k, p(s), None, None, None); samples.append(s)
    lib.ccm_sim3_solver_destroy(h)
    t_np = []
    for r in range(5):
        t0 = time.perf_counter()
        for pr, s in zip(problems, samples):
            ref.evaluate(pr, s)
        t_np.append(time.perf_counter() - t0)
    result = {"shape": {"candidates": a.candidates, "correspondences": a.n, "hypotheses": int(sum(n_hyp))},
              "first_return": {"candidate": hit[0], "turn": hit[1], "inliers": hit[2]} if hit else None,
              "create": stats(t_create), "create_round_robin_first_return_destroy": stats(t_first),
              "numpy_float64_all_hypotheses": stats(t_np)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    ctx.close()


if __name__ == "__main__":
    main()
