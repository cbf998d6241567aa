"""Local bundle adjustment at config 4 size (30 keyframes, 5,000 points, 40,000 observations): the array route a caller needs today
against ccm_ba_solve_table_frames on keyframe handles and the map-point table (include/ccm_hot.h "local BA on the table").

Routes, alternating inside one process after a warm-up (as tools/bench_tracking.py does), each timed with the host clock around work
that ends in a synchronisation; the table and the handles are put back to the start state, untimed, before every route:
  (A) widen keypoints, information values and positions from the float arrays the map holds to the doubles ccm_ba_solve takes,
      ccm_ba_solve (LocalBundleAdjustmentClient's schedule with the outlier flags), narrow the points, ccm_map_table_update(pos),
      ccm_frame_set_pose for every local keyframe, synchronise.  It runs twice per repetition (A1, A2): the spread between the two
      series is the yardstick for (B).
  (B) ccm_ba_solve_table_frames: everything read and written on the device, one download.
The LM loop is the same code in both.  Every repetition compares poses, outlier flags, table positions and handle poses bit for bit.
Output: profiles/<tag>_local_ba_table.json (medians, spread, bytes up / down counted from the shapes) and one summary line.

    python tools/bench_local_ba_table.py [--reps 30] [--warmup 5] [--tag mi355x] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import ba_table_case as B  # noqa: E402
from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.optimizer import Optimizer, pose_to_camera  # noqa: E402


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def traffic(Lst):
    """Bytes over PCIe per call, counted from the shapes.  `index` is what ccm_ba_solve uploads for any problem (vertex maps, the edge
    ends in device order, the two CSR structures) and both routes send alike."""
    P, L, E = Lst["P"], Lst["L"], Lst["E"]
    A = Lst["arrays"]
    free = A["fixed"] == 0
    nfree = int(free.sum()); e_free = int(free[A["edge_pose"]].sum()); n_local = int(Lst["publish"].sum())
    index = 4 * P + 4 * nfree + 8 * E + 4 * (L + 1) + 4 * (nfree + 1) + 4 * e_free
    a_up = 56 * P + 32 * P + 24 * L + 16 * E + 8 * E + index + (4 * L + 12 * L) + 96 * n_local
    a_down = 56 * P + 24 * L + E
    b_up = 56 * P + 32 * P + 4 * L + 4 * E + 32 * P + 4 * B.N_LEVELS + P + index
    b_down = 56 * P + E + 12 * L
    return {"index_bytes_both": index, "a_up": a_up, "a_down": a_down, "b_up": b_up, "b_down": b_down}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out", default=None, help="output file (default profiles/<tag>_local_ba_table.json)")
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    Lst = B.lists(B.graph("config4"))
    A = Lst["arrays"]
    ca, cb = B.Case(ctx, Lst), B.Case(ctx, Lst)
    # what the map holds: floats
    kx = A["obs"][:, 0].astype("f4"); ky = A["obs"][:, 1].astype("f4"); info32 = A["info"].astype("f4"); pos32 = A["points"].astype("f4")
    local = np.flatnonzero(Lst["publish"])
    all_slots = np.arange(Lst["capacity"], dtype="i4")

    def reset(case):
        case.table.update(all_slots, **Lst["rows"])
        for k, h in enumerate(case.kfs):
            h.set_pose(*case.cams[k])
        ctx.sync()

    def route_a():
        t0 = time.perf_counter()
        g = dict(A, obs=np.stack([kx, ky], 1).astype("f8"), info=info32.astype("f8"), points=pos32.astype("f8"))
        r = Optimizer.LocalBundleAdjustmentClient(g, ctx=ctx)
        ca.table.update(Lst["slot"], pos=r["points"].astype("f4"))
        for k in local:
            ca.kfs[k].set_pose(*pose_to_camera(r["poses"][k]))
        ctx.sync()
        return time.perf_counter() - t0, r

    def route_b():
        t0 = time.perf_counter()
        r = Optimizer.LocalBundleAdjustmentClientTable(cb.table, cb.kfs, Lst["table_lists"], ctx=ctx)
        return time.perf_counter() - t0, r

    def same(ra, rb):
        ok = ra["poses"].tobytes() == rb["poses"].tobytes() and ra["outlier"].tobytes() == rb["outlier"].tobytes()
        ok = ok and ca.table.fetch(Lst["slot"])["pos"].tobytes() == cb.table.fetch(Lst["slot"])["pos"].tobytes()
        ok = ok and rb["pos"].tobytes() == ra["points"].astype("f4").tobytes()
        for k in range(Lst["P"]):
            Ta, Oa = ca.kfs[k].pose(); Tb, Ob = cb.kfs[k].pose()
            ok = ok and Ta.tobytes() == Tb.tobytes() and Oa.tobytes() == Ob.tobytes()
        return bool(ok)

    for _ in range(a.warmup):
        reset(ca); route_a(); reset(cb); route_b()
    t_a1, t_a2, t_b, solve_a, solve_b = [], [], [], [], []
    mismatches = 0
    orders = (("a1", "b", "a2"), ("b", "a2", "a1"), ("a2", "a1", "b"))
    for rep in range(a.reps):
        ra = rb = None
        for which in orders[rep % 3]:
            if which == "b":
                reset(cb); t, rb = route_b(); t_b.append(t)
                solve_b.append(rb["t_linearize"] + rb["t_schur"] + rb["t_solve"] + rb["t_update"])
            else:
                reset(ca); t, ra = route_a(); (t_a1 if which == "a1" else t_a2).append(t)
                solve_a.append(ra["t_linearize"] + ra["t_schur"] + ra["t_solve"] + ra["t_update"])
        mismatches += not same(ra, rb)
    sa1, sa2, sb = stats(t_a1), stats(t_a2), stats(t_b)
    a_med = 0.5 * (sa1["median_ms"] + sa2["median_ms"])
    spread = abs(sa1["median_ms"] - sa2["median_ms"])
    res = {"workload": {"keyframes": Lst["P"], "points": Lst["L"], "observations": Lst["E"], "local_keyframes": int(len(local)),
                        "reps": a.reps, "warmup": a.warmup},
           "a1_array_route": sa1, "a2_array_route": sa2, "b_table_route": sb,
           "a_lm_loop": stats(solve_a), "b_lm_loop": stats(solve_b),
           "a_median_ms": round(a_med, 4), "a1_a2_spread_ms": round(spread, 4),
           "b_minus_a_ms": round(sb["median_ms"] - a_med, 4), "b_within_spread_or_faster": bool(sb["median_ms"] - a_med <= spread),
           "mismatching_reps": int(mismatches), "bytes": traffic(Lst)}
    out = a.out or os.path.join(ROOT, "profiles", "%s_local_ba_table.json" % a.tag)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("local BA config 4 | (A1) %.3f (A2) %.3f ms, spread %.3f | (B) table route %.3f ms | B - A = %+.3f ms | LM loop A %.3f B %.3f ms | "
          "up %d -> %d bytes, down %d -> %d | mismatches %d" % (
              sa1["median_ms"], sa2["median_ms"], spread, sb["median_ms"], res["b_minus_a_ms"], res["a_lm_loop"]["median_ms"],
              res["b_lm_loop"]["median_ms"], res["bytes"]["a_up"], res["bytes"]["b_up"], res["bytes"]["a_down"], res["bytes"]["b_down"], mismatches),
          flush=True)
    ca.close(); cb.close()
    return 1 if mismatches else 0


if __name__ == "__main__":
    sys.exit(main())
