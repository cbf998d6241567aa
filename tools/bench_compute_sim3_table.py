"""ComputeSim3's two matchers: the host projection and the array calls against the calls on keyframe handles and the map-point table
(include/ccm_hot.h "ComputeSim3 on keyframe handles and the table").

Sizes (scenes of tests/sim3_table_ref.py, synthetic features):
  sim3_1_pair    one candidate pair of 1,000 x 1,000 features, about 60 % of them holding points, th = 7.5
  sim3_3_pairs   three such pairs
  loop_1kf       one keyframe of 1,000 features x 4,000 loop points, th = 10
Routes, alternating inside one process after a warm-up, each timed with the host clock around work that ends in a synchronisation
(every C call returns after its download), the results compared after every repetition:
  (a) today's route: the host projection -- the numpy restatement of tests/sim3_table_ref.py standing in for the reference's per-point
      cv::Mat loop, which nobody has timed; timed separately -- then ccm_search_by_sim3 (once per pair) or
      ccm_search_by_projection_sim3_batch on the projected arrays (laid out before the clock starts: only the C call is timed)
  (b) ccm_search_by_sim3_table_frames / ccm_search_by_projection_table_frames (only the C call is timed; no taps)
The bar: at each size the median of (b) is at most the median of the array call of (a) alone plus the larger of 5 % and that call's
own p10-p90 spread.
Output: profiles/<tag>_sim3_table.json and one summary line.

    python tools/bench_compute_sim3_table.py [--reps 30] [--warmup 5] [--tag mi355x]
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
import sim3_table_ref as Q  # noqa: E402
from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.frame import DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher  # noqa: E402
from motioncheck_ccm_slam_amd.tracking import MapPointTable  # noqa: E402

seg = lambda b: (b + 63) // 64 * 64  # noqa: E731


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def view(kf):
    return FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"].reshape(-1, 32))


def table_of(ctx, sc):
    t = MapPointTable(sc["capacity"], ctx=ctx)
    live = np.flatnonzero(sc["rows"]["flags"] & R.LIVE)
    t.update(live, **{k: sc["rows"][k][live] for k in R.COLS})
    return t


def alternate(route_a, route_b, same, warmup, reps, clear):
    for _ in range(warmup):
        route_a(); route_b()
    clear()
    mismatches = 0
    for r in range(reps):
        if r % 2 == 0:
            route_a(); route_b()
        else:
            route_b(); route_a()
        mismatches += not same()
    return mismatches


def summary(name, extra, t_proj, t_a, t_b, a_up, b_up, mismatches):
    sa, sb = stats(t_a), stats(t_b)
    margin = max(0.05 * sa["median_ms"], sa["p90_ms"] - sa["p10_ms"])
    out = dict(extra, mismatching_reps=int(mismatches), a_host_projection_numpy=stats(t_proj), a_array_call=sa, b_table_frames_call=sb,
               a_upload_bytes=int(a_up), b_upload_bytes=int(b_up), ratio_a_call_over_b=round(sa["median_ms"] / sb["median_ms"], 3),
               margin_ms=round(margin, 4), b_within_bar=bool(sb["median_ms"] <= sa["median_ms"] + margin))
    print("%-12s (a) host projection %.3f ms + array call %.3f ms [%.3f, %.3f] | (b) %.3f ms [%.3f, %.3f] | a call / b = %.2f | upload %d -> %d bytes |"
          " mismatches %d" % (name, out["a_host_projection_numpy"]["median_ms"], sa["median_ms"], sa["p10_ms"], sa["p90_ms"], sb["median_ms"], sb["p10_ms"],
                              sb["p90_ms"], out["ratio_a_call_over_b"], a_up, b_up, mismatches), flush=True)
    return out


def bench_sim3(ctx, lib, n_pairs, a):
    p = _lib.ptr
    m = ORBmatcher(ctx=ctx)
    sc = Q.big_sim3_scene(lambda k: R.synthetic_features(1000, 300 + k), n_pairs)
    hs = {}
    for kf in sc["kfs"]:
        h = DeviceFrame(view(kf), None, ctx=ctx)
        h.map_points = kf["mp_id"]
        hs[id(kf)] = h
    table = table_of(ctx, sc)
    pairs = sc["pairs"]
    # once through the wrapper, with the taps: the device's level on ambiguous entries, so that both routes search the same windows
    res = m.SearchBySim3TableFrames(table, [dict(q, kf1=hs[id(q["kf1"])], kf2=hs[id(q["kf2"])]) for q in pairs], Q.SCALE, th=7.5,
                                    log_scale_factor1=Q.LOG_SF, taps=True)
    gates_equal, levels, n_amb = True, [], 0
    for k, q in enumerate(pairs):
        ds = Q.sim3_pair(sc, q)
        gates_equal &= all(bool((res["gate" + d][k] == g["gate"]).all()) for d, g in zip("12", ds))
        levels.append([np.ascontiguousarray(np.where(g["ambiguous"], res["level" + d][k], g["level"]), "i4") for d, g in zip("12", ds)])
        n_amb += sum(int(g["ambiguous"].sum()) for g in ds)
    recs = (_lib.Sim3SearchPair * n_pairs)()
    keep = []
    n1 = [len(q["kf1"]["kx"]) for q in pairs]
    for k, q in enumerate(pairs):
        rec = recs[k]
        rec.kf1 = hs[id(q["kf1"])].handle; rec.kf2 = hs[id(q["kf2"])].handle
        for name in ("T1w", "T2w", "S21", "S12"):
            getattr(rec, name)[:] = [float(x) for x in np.asarray(q[name], "f4").reshape(12)]
        rec.fx, rec.fy, rec.cx, rec.cy = [float(x) for x in q["intr"]]
        rec.bounds1[:] = [float(x) for x in q["bounds1"]]; rec.bounds2[:] = [float(x) for x in q["bounds2"]]
        keep += [np.ascontiguousarray(q["matched12"], "i4"), np.ascontiguousarray(q["matched_idx2"], "i4")]
        rec.matched12 = p(keep[-2]); rec.matched_idx2 = p(keep[-1])
    prob = _lib.Sim3SearchProblem(n_pairs, recs, 7.5, float(Q.LOG_SF), Q.N_LEVELS, p(Q.SCALE), float(Q.LOG_SF), Q.N_LEVELS, p(Q.SCALE))
    b_m12 = np.empty(sum(n1), "i4"); b_found = np.zeros(n_pairs, "i4")
    rb = _lib.Sim3SearchResult(p(b_m12), p(b_found), *([None] * 10))
    a_m12 = [np.empty(n, "i4") for n in n1]
    host = [(view(q["kf1"]), view(q["kf2"])) for q in pairs]                  # the array route's keyframes: host arrays, kept alive here
    grids = [(v1.struct(), v2.struct()) for v1, v2 in host]
    t_proj, t_a, t_b = [], [], []
    state = {}

    def route_a():
        t0 = time.perf_counter()
        proj = [Q.sim3_pair(sc, q) for q in pairs]
        t1 = time.perf_counter()
        args = []
        for k, (d1, d2) in enumerate(proj):
            args.append([np.ascontiguousarray(x) for x in (
                (d1["gate"] == Q.SEARCHED).astype(np.uint8), d1["u"], d1["v"], levels[k][0], d1["desc"],
                (d2["gate"] == Q.SEARCHED).astype(np.uint8), d2["u"], d2["v"], levels[k][1], d2["desc"])])
        t2 = time.perf_counter()
        total = 0
        for k in range(n_pairs):
            total += ctx.check(lib.ccm_search_by_sim3(ctx.handle, C.byref(grids[k][0]), p(Q.SCALE), C.byref(grids[k][1]), p(Q.SCALE),
                                                      *[p(x) for x in args[k]], C.c_float(7.5), p(a_m12[k])))
        t3 = time.perf_counter()
        t_proj.append(t1 - t0); t_a.append(t3 - t2)
        state["a_total"] = total
        state["searched"] = int(sum(x[0].sum() + x[5].sum() for x in args))

    def route_b():
        t0 = time.perf_counter()
        state["b_total"] = ctx.check(lib.ccm_search_by_sim3_table_frames(ctx.handle, C.c_void_p(table.handle), C.byref(prob), C.byref(rb)))
        t_b.append(time.perf_counter() - t0)

    def same():
        return state["a_total"] == state["b_total"] and np.concatenate(a_m12).tobytes() == b_m12.tobytes()

    mismatches = alternate(route_a, route_b, same, a.warmup, a.reps, lambda: [v.clear() for v in (t_proj, t_a, t_b)])
    # host-to-device bytes: (a) per pair two keyframes' features (x, y, octave, descriptor: 44 bytes each) and grids, and per feature of either
    # side a query (valid is folded into the radius: x, y, r, two levels and a descriptor, 52 bytes); (b) the staging copy of mpt_sim3_host.cpp
    n2 = [len(q["kf2"]["kx"]) for q in pairs]
    a_up = sum((x + y) * (44 + 52) for x, y in zip(n1, n2))
    b_up = seg(2 * n_pairs * 168) + seg(2 * n_pairs * 80) + seg(n_pairs * 16) + 2 * seg(sum(n1) * 4)
    out = summary("sim3_%d_pair%s" % (n_pairs, "s" if n_pairs > 1 else ""), dict(pairs=n_pairs, features=[n1, n2], searched=state["searched"],
                  found=int(state["b_total"]), ambiguous=n_amb, gates_equal_restatement=bool(gates_equal), th=7.5), t_proj, t_a, t_b, a_up, b_up, mismatches)
    for h in hs.values():
        h.close()
    table.close()
    return out, mismatches + (not gates_equal)


def bench_loop(ctx, lib, a):
    p = _lib.ptr
    m = ORBmatcher(ctx=ctx)
    sc = Q.big_loop_scene()
    kf = sc["kfs"][0]
    h = DeviceFrame(view(kf), None, ctx=ctx)
    h.map_points = kf["mp_id"]
    table = table_of(ctx, sc)
    n, N = len(sc["slots"]), len(kf["kx"])
    res = m.SearchByProjectionTableFrames(table, [h], [kf["Tcw"]], [kf["Ow"]], R.INTR, R.BOUNDS, sc["slots"], [kf["matched_slot"]], Q.SCALE, th=10.0,
                                          log_scale_factor=Q.LOG_SF, taps=True)
    g = Q.loop_views(sc)
    gates_equal = bool((res["gate"] == g["gate"]).all())
    level = np.ascontiguousarray(np.where(g["ambiguous"], res["level"], g["level"])[0], "i4")
    slots = np.ascontiguousarray(sc["slots"], "i4"); ms_in = np.ascontiguousarray(kf["matched_slot"], "i4")
    views = (_lib.LoopView * 1)()
    V = views[0].view
    V.kf = h.handle
    V.Tcw[:] = [float(x) for x in kf["Tcw"].reshape(-1)]; V.Ow[:] = [float(x) for x in kf["Ow"]]
    V.fx, V.fy, V.cx, V.cy = R.INTR
    V.min_x, V.max_x, V.min_y, V.max_y = R.BOUNDS
    views[0].matched_slot = p(ms_in)
    prob = _lib.LoopProjectionProblem(1, views, n, p(slots), float(Q.LOG_SF), Q.N_LEVELS, p(Q.SCALE), 10.0)
    b_idx = np.empty(n, "i4"); b_obs = np.empty(n, np.uint8); b_ms = np.empty(N, "i4"); b_nm = np.zeros(1, "i4")
    rb = _lib.LoopProjectionResult(p(b_idx), p(b_obs), p(b_ms), p(b_nm), None, None, None, None, None)
    a_idx = np.empty(n, "i4"); a_nm = np.zeros(1, "i4")
    keep = view(kf)                                                            # the array route's keyframe: host arrays, kept alive here
    grid = (_lib.FrameGrid * 1)(keep.struct())
    first = np.array([0, n], "i4")
    desc = np.ascontiguousarray(sc["rows"]["desc"][slots])
    t_proj, t_a, t_b = [], [], []
    state = {}

    def route_a():
        t0 = time.perf_counter()
        gg = Q.loop_views(sc)
        t1 = time.perf_counter()
        valid = np.ascontiguousarray(gg["gate"][0] == Q.LG_SEARCHED, np.uint8)
        uu = np.ascontiguousarray(gg["u"][0]); vv = np.ascontiguousarray(gg["v"][0]); ob = np.ascontiguousarray(gg["observed"][0], np.uint8)
        mt = np.ascontiguousarray(ms_in >= 0, np.uint8)
        t2 = time.perf_counter()
        state["a_total"] = ctx.check(lib.ccm_search_by_projection_sim3_batch(ctx.handle, 1, C.cast(grid, C.c_void_p), p(Q.SCALE), p(first), p(valid), p(uu),
                                                                             p(vv), p(level), p(desc), p(ob), p(mt), C.c_float(10.0), p(a_idx), p(a_nm)))
        t3 = time.perf_counter()
        t_proj.append(t1 - t0); t_a.append(t3 - t2)
        state["a_matched"] = mt; state["searched"] = int(valid.sum())

    def route_b():
        t0 = time.perf_counter()
        state["b_total"] = ctx.check(lib.ccm_search_by_projection_table_frames(ctx.handle, C.c_void_p(table.handle), C.byref(prob), C.byref(rb)))
        t_b.append(time.perf_counter() - t0)

    def same():
        return state["a_total"] == state["b_total"] and a_idx.tobytes() == b_idx.tobytes() and ((b_ms >= 0) == (state["a_matched"] != 0)).all()

    mismatches = alternate(route_a, route_b, same, a.warmup, a.reps, lambda: [v.clear() for v in (t_proj, t_a, t_b)])
    # (a) the keyframe's features and grid, and per point x, y, r, two levels, the keyframe index, the level (28 bytes), valid and observed, a descriptor;
    # the vpMatched flags; (b) the staging copy of mpt_sim3_host.cpp
    a_up = N * 44 + 80 + n * (28 + 2 + 32) + N + 16
    b_up = seg(112) + seg(80) + seg(16) + seg(4) + seg(n * 4) + seg(N * 4)
    out = summary("loop_1kf", dict(keyframes=1, features=N, points=n, searched=state["searched"], matches=int(state["b_total"]),
                                   ambiguous=int(g["ambiguous"].sum()), gates_equal_restatement=gates_equal, th=10.0), t_proj, t_a, t_b, a_up, b_up, mismatches)
    del keep
    h.close(); table.close()
    return out, mismatches + (not gates_equal)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out", default=None, help="output file (default profiles/<tag>_sim3_table.json)")
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    lib = _lib.load()
    result = {"workload": {"reps": a.reps, "warmup": a.warmup}, "sizes": {}}
    bad = 0
    for name, fn in (("sim3_1_pair", lambda: bench_sim3(ctx, lib, 1, a)), ("sim3_3_pairs", lambda: bench_sim3(ctx, lib, 3, a)),
                     ("loop_1kf", lambda: bench_loop(ctx, lib, a))):
        out, b = fn()
        result["sizes"][name] = out
        bad += int(b)
    path = a.out or os.path.join(ROOT, "profiles", "%s_sim3_table.json" % a.tag)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: (v["a_array_call"]["median_ms"], v["b_table_frames_call"]["median_ms"], v["ratio_a_call_over_b"], v["b_within_bar"],
                          v["mismatching_reps"]) for k, v in result["sizes"].items()}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
