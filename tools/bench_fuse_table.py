"""ORBmatcher::Fuse up to the selection for one list of map points in many keyframes: host projection and
ccm_fuse_select_batch_frames against ccm_fuse_select_table_frames on the map-point table (include/ccm_hot.h "map-point table").

Two sizes, keyframes of 1,000 synthetic features (tests/fuse_table_ref.py make_scene):
  loop_closing   40 keyframes x 4,000 points   (LoopFinder / MapMerger SearchAndFuse: chi2_check = 0, th = 4)
  local_mapping  20 keyframes x 1,000 points   (the first loop of SearchInNeighbors: chi2_check = 1, th = 3)
Routes, alternating inside one process after a warm-up, each timed with the host clock around work that ends in a synchronisation
(both C calls return after their download), best_idx / best_dist compared after every repetition:
  (a) today's route: the host projection -- tests/fuse_table_ref.py fuse_gates, numpy vectorised over the points, standing in for the
      reference's per-point cv::Mat loop; timed separately -- then ccm_fuse_select_batch_frames on the valid / u / v / level arrays and
      one 32-byte descriptor per pair (the arrays are laid out before the clock starts: only the C call is timed)
  (b) ccm_fuse_select_table_frames (only the C call is timed; best_idx and best_dist, no taps)
The bar: at the loop-closing size the median of (b) is at most the median of the ccm_fuse_select_batch_frames call of (a) alone plus
the larger of 5 % and that call's own p10-p90 spread.
Output: profiles/<tag>_fuse_table.json and one summary line.

    python tools/bench_fuse_table.py [--reps 30] [--warmup 5] [--tag mi355x]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import fuse_table_ref as R  # noqa: E402
import search_local_points_ref as S  # noqa: E402
from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.frame import DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import FrameGridView  # noqa: E402
from motioncheck_ccm_slam_amd.tracking import MapPointTable  # noqa: E402

N_FEAT = 1000


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def workload(n_kf, n_points, seed):
    """n_kf cameras scattered round tests' camera, 1,000 synthetic features each; 60 % of the points are back-projected features
    (equal shares per keyframe, a fifth of each share already held by its keyframe), the rest random distractors."""
    rng = np.random.default_rng(seed)
    cams = [S.camera(tuple(rng.normal(0, 0.04, 3)), tuple(np.array([2.5, -1.5, 1.5]) + rng.normal(0, 0.4, 3))) for _ in range(n_kf)]
    n_match = int(0.6 * n_points / n_kf)
    return R.make_scene([R.synthetic_features(N_FEAT, seed + 1 + k) for k in range(n_kf)], n_points, n_match, n_match // 5, seed=seed, cams=cams)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out", default=None, help="output file (default profiles/<tag>_fuse_table.json)")
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    lib = _lib.load()
    p = _lib.ptr
    result = {"workload": {"features": N_FEAT, "reps": a.reps, "warmup": a.warmup}, "sizes": {}}
    bad = 0
    for name, n_kf, n_points, par in (("loop_closing", 40, 4000, R.PARAMS[1]), ("local_mapping", 20, 1000, R.PARAMS[0])):
        sc = workload(n_kf, n_points, 11)
        kfs = sc["kfs"]
        handles = []
        for kf in kfs:
            h = DeviceFrame(FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"]), None, ctx=ctx)
            h.map_points = kf["mp_id"]
            handles.append(h)
        table = MapPointTable(sc["capacity"], ctx=ctx)
        live = np.flatnonzero(sc["rows"]["flags"] & R.LIVE)
        table.update(live, **{k: sc["rows"][k][live] for k in R.COLS})
        m = n_kf * n_points
        harr = (C.c_void_p * n_kf)(*[h.handle for h in handles])
        first = (np.arange(n_kf + 1) * n_points).astype("i4")
        slots = np.ascontiguousarray(sc["slots"], "i4")
        desc = np.ascontiguousarray(np.tile(sc["rows"]["desc"][slots], (n_kf, 1)))           # route (a): one descriptor per pair
        views = (_lib.FuseView * n_kf)()
        for k, kf in enumerate(kfs):
            views[k].kf = handles[k].handle
            views[k].Tcw[:] = [float(x) for x in kf["Tcw"].reshape(-1)]; views[k].Ow[:] = [float(x) for x in kf["Ow"]]
            views[k].fx, views[k].fy, views[k].cx, views[k].cy = R.INTR
            views[k].min_x, views[k].max_x, views[k].min_y, views[k].max_y = R.BOUNDS
        prob = _lib.FuseTableProblem(n_kf, views, n_points, p(slots), None, float(R.LOG_SF), R.N_LEVELS, p(R.SCALE), p(R.INV_SIGMA2), float(par["th"]),
                                     int(par["chi2_check"]), int(par["accept_th"]))
        b_idx = np.empty(m, "i4"); b_dist = np.empty(m, "i4"); b_gate = np.empty(m, np.uint8); b_u = np.empty(m, "f4"); b_v = np.empty(m, "f4")
        b_lvl = np.empty(m, "i4")
        a_idx = np.empty(m, "i4"); a_dist = np.empty(m, "i4")
        # once, with the taps: the device's level on the pairs the restatement calls ambiguous, so that both routes search the same windows
        res = _lib.FuseTableResult(p(b_idx), p(b_dist), p(b_gate), p(b_u), p(b_v), p(b_lvl), 0)
        ctx.check(lib.ccm_fuse_select_table_frames(ctx.handle, C.c_void_p(table.handle), C.byref(prob), C.byref(res)))
        g = R.fuse_gates(sc)
        gates_equal = bool((g["gate"].ravel() == b_gate).all())
        amb = g["ambiguous"].ravel()
        level = np.ascontiguousarray(np.where(amb, b_lvl, g["level"].ravel()), "i4")
        res = _lib.FuseTableResult(p(b_idx), p(b_dist), None, None, None, None, 0)
        t_proj, t_a, t_b = [], [], []
        state = {}

        def route_a():
            t0 = time.perf_counter()
            gg = R.fuse_gates(sc)
            t1 = time.perf_counter()
            valid = np.ascontiguousarray((gg["gate"] == R.SEARCHED).ravel(), np.uint8)
            uu = np.ascontiguousarray(gg["u"].ravel()); vv = np.ascontiguousarray(gg["v"].ravel())
            t2 = time.perf_counter()
            ctx.check(lib.ccm_fuse_select_batch_frames(ctx.handle, n_kf, harr, p(R.SCALE), p(R.INV_SIGMA2), p(first), p(valid), p(uu), p(vv), p(level),
                                                       p(desc), C.c_float(par["th"]), int(par["chi2_check"]), int(par["accept_th"]), p(a_idx), p(a_dist)))
            t3 = time.perf_counter()
            t_proj.append(t1 - t0); t_a.append(t3 - t2)
            state["searched"] = int(valid.sum())

        def route_b():
            t0 = time.perf_counter()
            ctx.check(lib.ccm_fuse_select_table_frames(ctx.handle, C.c_void_p(table.handle), C.byref(prob), C.byref(res)))
            t_b.append(time.perf_counter() - t0)

        for _ in range(a.warmup):
            route_a(); route_b()
        for v in (t_proj, t_a, t_b):
            v.clear()
        mismatches = 0
        for r in range(a.reps):
            a_idx.fill(-7); b_idx.fill(-9)
            if r % 2 == 0:
                route_a(); route_b()
            else:
                route_b(); route_a()
            mismatches += not ((a_idx == b_idx).all() and (a_dist == b_dist).all())
        sa, sb = stats(t_a), stats(t_b)
        # host-to-device bytes by the two calls' own layouts (match_window_host.cpp fuse_batch_run; mpt_fuse_host.cpp, whose static_assert pins the
        # 112-byte view and the 80-byte grid record per keyframe, every segment of the staging copy rounded up to 64 bytes)
        seg = lambda b: (b + 63) // 64 * 64  # noqa: E731
        chi2 = int(par["chi2_check"])
        a_up = m * (6 * 4 + 32) + n_kf * 80 + chi2 * R.N_LEVELS * 4      # qx qy qr minl maxl q_kf, a descriptor per pair; the grid records
        b_up = seg(n_kf * 112) + seg(n_kf * 80) + seg(n_points * 4) + chi2 * 64
        margin = max(0.05 * sa["median_ms"], sa["p90_ms"] - sa["p10_ms"])
        out = {"keyframes": n_kf, "points": n_points, "pairs": m, "searched_pairs": state["searched"], "accepted": int((b_idx >= 0).sum()),
               "ambiguous_pairs": int(amb.sum()), "gates_equal_restatement": gates_equal, "params": {k: (float(v) if k == "th" else int(v)) for k, v in par.items()},
               "mismatching_reps": int(mismatches), "a_host_projection_numpy": stats(t_proj), "a_fuse_select_batch_frames": sa,
               "b_fuse_select_table_frames": sb, "a_upload_bytes": a_up, "b_upload_bytes": b_up,
               "ratio_a_call_over_b": round(sa["median_ms"] / sb["median_ms"], 3), "margin_ms": round(margin, 4),
               "b_within_bar": bool(sb["median_ms"] <= sa["median_ms"] + margin)}
        result["sizes"][name] = out
        bad += mismatches + (not gates_equal)
        print("%-13s %2d kf x %4d points = %6d pairs, %6d searched | (a) host projection %.3f ms + select_batch_frames %.3f ms [%.3f, %.3f] |"
              " (b) select_table_frames %.3f ms [%.3f, %.3f] | a call / b = %.2f | mismatches %d" % (
                  name, n_kf, n_points, m, state["searched"], out["a_host_projection_numpy"]["median_ms"], sa["median_ms"], sa["p10_ms"], sa["p90_ms"],
                  sb["median_ms"], sb["p10_ms"], sb["p90_ms"], out["ratio_a_call_over_b"], mismatches), flush=True)
        for h in handles:
            h.close()
        table.close()
    path = a.out or os.path.join(ROOT, "profiles", "%s_fuse_table.json" % a.tag)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: (v["a_fuse_select_batch_frames"]["median_ms"], v["b_fuse_select_table_frames"]["median_ms"], v["ratio_a_call_over_b"],
                          v["b_within_bar"], v["mismatching_reps"]) for k, v in result["sizes"].items()}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
