#!/usr/bin/env python3
"""LocalMapping::CreateNewMapPoints: one batched call against the per-neighbour path (include/ccm_hot.h "CreateNewMapPoints").

Workload: the scene of tests/create_new_map_points_ref.make_scene with 20 neighbours and about 2000 features per keyframe.  Two
paths on the same host buffers and a third on keyframe handles, alternating inside one process after a warm-up, each timed with the host clock around calls that end
with a stream synchronisation:
  (a) the per-neighbour path: one ccm_search_for_triangulation per neighbour the baseline rule keeps (19 of 20), one after the
      other.  This is the MATCHING half only; the triangulation of its pairs is not part of it.
  (b) one ccm_create_new_map_points: matching against all 20 neighbours, triangulation, gates and the ordered resolution.
  (c) one ccm_create_new_map_points_frames on keyframe handles made once, outside the timed region.  Inside the timed region one
      neighbour's mp_id and pose are sent again per repetition (ccm_frame_set_map_points, ccm_frame_set_pose), which is what a real
      keyframe step costs.
Every repetition compares them: each row (kf, idx1, idx2) of (b)'s list must be (a)'s match of idx1 in neighbour kf, and (c)'s
n_new, kf, idx1, idx2, x3d and first must be (b)'s bytes.
ctypes argument lists are built once; what is timed is the C call.

With --kernel-stats FILE (the kernel statistics CSV of a separate run under `rocprofv3 --kernel-trace --stats`) the durations of
k_cnmp_match, k_cnmp_triangulate, k_cnmp_resolve, their _frames variants and k_hamming_ranges are added.
Output: profiles/<tag>_create_new_map_points.json and one summary line.

    python tools/bench_create_new_map_points.py [--reps 200] [--warmup 20] [--tag mi355x]
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (first, so that the library binds to the same HIP runtime as in the tests)

from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.frame import DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.mapping import MapKeyFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import FrameGridView  # noqa: E402
import create_new_map_points_ref as ref  # noqa: E402

KERNELS = ("k_cnmp_match_frames", "k_cnmp_triangulate_frames", "k_cnmp_resolve_frames", "k_cnmp_match", "k_cnmp_triangulate", "k_cnmp_resolve",
           "k_hamming_ranges", "k_frame_kf_gather")


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def kernel_stats(path):
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if re.search(r"\b%s\b" % k, row["Name"]):
                    out[k] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=2300, help="3-D points of the scene (about 0.9 of them are seen by a keyframe)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--kernel-stats", default=None, metavar="FILE")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.init()
    ctx = _lib.Context(0); lib = ctx.lib; p = _lib.ptr
    sc = ref.make_scene(n_points=a.points, n_kf=20)
    curd, nbd = sc["current"], sc["neighbours"]
    mk = lambda d: MapKeyFrame(d["kp_x"], d["kp_y"], d["kp_octave"], d["desc"], d["node"], d["has_mp"], d["K"], d["Tcw"], d["Ow"],
                               d["scale_factors"], d["level_sigma2"])
    cur = mk(curd); nbs = [mk(d) for d in nbd]
    n1, n_kf = cur.n, len(nbs)
    epi = np.array([ref.epipole32(curd, d) for d in nbd], "f4")
    F12 = np.ascontiguousarray(sc["F12"], "f4"); md = np.ascontiguousarray(sc["median_depth"], "f4")
    kept = [k for k in range(n_kf) if not ref.baseline_too_short(curd["Ow"], nbd[k]["Ow"], md[k])]

    # (a): argument lists of the per-neighbour calls
    ang1 = np.zeros(n1, "f4"); match_a = np.full((n_kf, n1), -1, "i4")
    keep = [ang1]
    calls = []
    for k in kept:
        kf = nbs[k]
        ang2 = np.zeros(kf.n, "f4"); keep.append(ang2)
        calls.append((ctx.handle, p(cur.desc), p(cur.node), p(cur.has_mp), p(cur.kp_x), p(cur.kp_y), p(ang1), n1, p(kf.desc), p(kf.node), p(kf.has_mp),
                      p(kf.kp_x), p(kf.kp_y), p(ang2), p(kf.kp_octave), kf.n, p(F12[k]), C.c_float(epi[k, 0]), C.c_float(epi[k, 1]),
                      p(kf.scale_factors), p(kf.level_sigma2), 0, p(match_a[k])))

    def path_a():
        for args in calls:
            ctx.check(lib.ccm_search_for_triangulation(*args))

    # (b): the structures of the one call
    cs = cur.as_struct(); arr = (_lib.MapKeyframe * n_kf)(*[k.as_struct() for k in nbs])
    pb = _lib.NewPointsProblem(C.pointer(cs), n_kf, arr, p(F12), p(epi), p(md))
    o = dict(kf=np.zeros(n1, "i4"), idx1=np.zeros(n1, "i4"), idx2=np.zeros(n1, "i4"), x3d=np.zeros((n1, 3), "f4"), first=np.zeros(n_kf + 1, "i4"))
    res = _lib.NewPointsResult(0, p(o["kf"]), p(o["idx1"]), p(o["idx2"]), p(o["x3d"]), p(o["first"]), None)

    def path_b():
        return ctx.check(lib.ccm_create_new_map_points(ctx.handle, C.byref(pb), C.byref(res)))

    # (c): keyframe handles, made once
    def handle(d):
        f = DeviceFrame(FrameGridView(d["kp_x"], d["kp_y"], d["kp_octave"], d["desc"]), ctx=ctx)
        f.map_points = np.where(d["has_mp"] != 0, np.arange(len(d["has_mp"])), -1).astype("i4")
        f.set_camera(d["K"], d["scale_factors"], d["level_sigma2"]); f.set_bow(d["node"]); f.set_pose(d["Tcw"], d["Ow"])
        return f
    hcur = handle(curd); hnb = [handle(d) for d in nbd]
    harr = (C.c_void_p * n_kf)(*[f.handle for f in hnb])
    pbf = _lib.NewPointsFrames(hcur.handle, n_kf, harr, p(F12), p(epi), p(md))
    oc = {k: np.zeros_like(v) for k, v in o.items()}
    resc = _lib.NewPointsResult(0, p(oc["kf"]), p(oc["idx1"]), p(oc["idx2"]), p(oc["x3d"]), p(oc["first"]), None)
    ids = [np.where(d["has_mp"] != 0, np.arange(len(d["has_mp"])), -1).astype("i4") for d in nbd]
    pose = [(np.ascontiguousarray(d["Tcw"], "f4").reshape(12), np.ascontiguousarray(d["Ow"], "f4")) for d in nbd]

    def path_c(r):
        k = r % n_kf                                                          # the neighbour whose state is sent again (unchanged values)
        h = C.c_void_p(hnb[k].handle)
        ctx.check(lib.ccm_frame_set_map_points(h, p(ids[k])))
        ctx.check(lib.ccm_frame_set_pose(h, p(pose[k][0]), p(pose[k][1])))
        return ctx.check(lib.ccm_create_new_map_points_frames(ctx.handle, C.byref(pbf), C.byref(resc)))

    for r in range(a.warmup):
        path_a(); path_b(); path_c(r)
    t_a, t_b, t_c, mismatches, mismatches_c, n_new = [], [], [], 0, 0, 0
    for r in range(a.reps):
        for which in ((0, 1, 2), (1, 2, 0), (2, 0, 1))[r % 3]:                # rotate which path goes first
            t0 = time.perf_counter()
            if which == 0:
                path_a()
            elif which == 1:
                n_new = path_b()
            else:
                n_c = path_c(r)
            (t_a, t_b, t_c)[which].append(time.perf_counter() - t0)
        rows = slice(0, n_new)
        mismatches += not bool((match_a[o["kf"][rows], o["idx1"][rows]] == o["idx2"][rows]).all() and o["first"][n_kf] == n_new)
        mismatches_c += not (n_c == n_new and oc["first"].tobytes() == o["first"].tobytes() and
                             all(oc[k][rows].tobytes() == o[k][rows].tobytes() for k in ("kf", "idx1", "idx2", "x3d")))
    result = {"workload": {"features_current": n1, "features_neighbours": [k.n for k in nbs], "neighbours": n_kf, "neighbours_kept": len(kept),
                           "matches_a": int((match_a >= 0).sum()), "new_points_b": int(n_new), "reps": a.reps, "warmup": a.warmup},
              "a_sequential_search_for_triangulation": stats(t_a), "b_create_new_map_points": stats(t_b), "c_create_new_map_points_frames": stats(t_c),
              "mismatching_reps": int(mismatches), "c_reps_differing_from_b": int(mismatches_c)}
    if a.kernel_stats:
        result["kernels"] = kernel_stats(a.kernel_stats)
    out = a.out or os.path.join(ROOT, "profiles", "%s_create_new_map_points.json" % a.tag)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    for f in [hcur] + hnb:
        f.close()
    ctx.close()
    return 1 if mismatches or mismatches_c else 0


if __name__ == "__main__":
    sys.exit(main())
