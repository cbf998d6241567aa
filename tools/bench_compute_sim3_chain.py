"""ComputeSim3 from SearchBySim3 to OptimizeSim3's verdict: the links called one by one against the chain call
(include/ccm_hot.h "ComputeSim3 on handles: the solver, OptimizeSim3 and the chain").

Sizes: 1, 3 and 8 candidate pairs of 1,000 x 1,000 synthetic features, about 60 % of them holding points (tests/sim3_table_ref.py
big_sim3_scene), 20 entry marks per pair, gScm = the true Sim3 slightly off, th2 = 10.
Routes, alternating inside one process after a warm-up, each timed with the host clock around work that ends in a synchronisation,
the results compared after every repetition (match12, sim3, n_inliers and pruned, byte for byte):
  (a) ccm_search_by_sim3_table_frames; then the host list -- the filter of src/Optimizer.cpp:920-957 over the downloaded match12 and
      the six arrays of ccm_optimize_sim3, in vectorised numpy standing in for the reference's C++ loop, timed separately; then
      ccm_optimize_sim3
  (b) ccm_compute_sim3_table_frames (no taps)
There is no bar; (b) is compared with the two C calls of (a) alone, the host list left out of it.
Output: profiles/<tag>_sim3_chain.json and one summary line.

    python tools/bench_compute_sim3_chain.py [--reps 30] [--warmup 5] [--tag mi355x]
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

import compute_sim3_ref as X  # noqa: E402
import fuse_table_ref as R  # noqa: E402
import sim3_table_ref as Q  # noqa: E402
from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.frame import DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import FrameGridView, _fill_search_pair  # noqa: E402
from motioncheck_ccm_slam_amd.tracking import MapPointTable  # noqa: E402

seg = lambda b: (b + 63) // 64 * 64  # noqa: E731


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def host_list(sc, q, m12):
    """compute_sim3_ref.correspondences, vectorised."""
    fl = sc["rows"]["flags"]; cap = sc["capacity"]
    id1, id2 = q["kf1"]["mp_id"], q["kf2"]["mp_id"]
    i2 = np.where(q["matched12"] >= 0, q["matched_idx2"], m12)
    ok = (i2 >= 0) & (i2 < len(id2))
    s1 = id1; s2 = id2[np.where(ok, i2, 0)]
    for s in (s1, s2):
        inside = (s >= 0) & (s < cap)
        f = fl[np.where(inside, s, 0)]
        ok &= inside & ((f & X.LIVE) != 0) & ((f & X.BAD) == 0)
    i1 = np.flatnonzero(ok)
    return np.stack([i1, i2[i1]], 1).astype("i4")


def bench(ctx, lib, n_pairs, a):
    p = _lib.ptr
    sc = Q.big_sim3_scene(lambda k: R.synthetic_features(1000, 300 + k), n_pairs)
    rng = np.random.default_rng(n_pairs)
    hs = {}
    for kf in sc["kfs"]:
        h = DeviceFrame(FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"].reshape(-1, 32)), None, ctx=ctx)
        h.map_points = kf["mp_id"]
        hs[id(kf)] = h
    table = MapPointTable(sc["capacity"], ctx=ctx)
    live = np.flatnonzero(sc["rows"]["flags"] & R.LIVE)
    table.update(live, **{k: sc["rows"][k][live] for k in R.COLS})
    pairs = sc["pairs"]
    for q in pairs:
        q["sim3"] = X.true_sim3(q, rng, rot=0.002, trans=0.01)
    n1 = [len(q["kf1"]["kx"]) for q in pairs]
    sum1 = sum(n1); f1 = np.concatenate([[0], np.cumsum(n1)]).astype(int)
    srec = (_lib.Sim3SearchPair * n_pairs)(); crec = (_lib.ComputeSim3Pair * n_pairs)()
    keep = []
    for k, q in enumerate(pairs):
        for rec in (srec[k], crec[k].search):
            _fill_search_pair(rec, dict(q, kf1=hs[id(q["kf1"])], kf2=hs[id(q["kf2"])]), n1[k], keep)
        crec[k].K2[:] = [float(x) for x in q["intr"]]; crec[k].sim3[:] = [float(x) for x in q["sim3"]]; crec[k].fix_scale = 0; crec[k].th2 = 10.0
    sprob = _lib.Sim3SearchProblem(n_pairs, srec, 7.5, float(Q.LOG_SF), Q.N_LEVELS, p(Q.SCALE), float(Q.LOG_SF), Q.N_LEVELS, p(Q.SCALE))
    cprob = _lib.ComputeSim3Problem(n_pairs, crec, 7.5, float(Q.LOG_SF), Q.N_LEVELS, p(Q.SCALE), p(X.INV_SIGMA2), float(Q.LOG_SF), Q.N_LEVELS, p(Q.SCALE),
                                    p(X.INV_SIGMA2))
    a_m12 = np.empty(sum1, "i4"); a_found = np.zeros(n_pairs, "i4")
    ra = _lib.Sim3SearchResult(p(a_m12), p(a_found), *([None] * 10))
    b_m12 = np.empty(sum1, "i4"); b_found = np.zeros(n_pairs, "i4"); b_pruned = np.zeros(sum1, np.uint8); b_nc = np.zeros(n_pairs, "i4")
    b_nin = np.zeros(n_pairs, "i4"); b_s3 = np.zeros((n_pairs, 8), "f8")
    rb = _lib.ComputeSim3Result(_lib.Sim3SearchResult(p(b_m12), p(b_found), *([None] * 10)), p(b_pruned), p(b_nc), p(b_nin), p(b_s3), None, None)
    K = np.array([q["intr"] for q in pairs], "f4").astype("f8"); fix = np.zeros(n_pairs, "i4"); th2 = np.full(n_pairs, 10.0, "f4")
    S0 = np.stack([q["sim3"] for q in pairs])
    t_search, t_list, t_opt, t_b = [], [], [], []
    state = {}

    def route_a():
        t0 = time.perf_counter()
        state["a_total"] = ctx.check(lib.ccm_search_by_sim3_table_frames(ctx.handle, C.c_void_p(table.handle), C.byref(sprob), C.byref(ra)))
        t1 = time.perf_counter()
        corr = [host_list(sc, q, a_m12[f1[k]:f1[k + 1]]) for k, q in enumerate(pairs)]
        A = [X.opt_arrays(sc["rows"], q, c[:, 0], c[:, 1]) for q, c in zip(pairs, corr)]
        cat = [np.ascontiguousarray(np.concatenate([x[key] for x in A])) for key in ("P1", "P2", "obs1", "obs2", "info1", "info2")]
        first = np.concatenate([[0], np.cumsum([len(c) for c in corr])]).astype("i4")
        s3 = S0.copy(); inl = np.zeros(max(int(first[-1]), 1), np.uint8); nin = np.zeros(n_pairs, "i4")
        pb = _lib.Sim3Problem(n_pairs, p(s3), p(fix), p(K), p(K), p(first), *[p(x) for x in cat], p(th2), p(inl), p(nin))
        t2 = time.perf_counter()
        ctx.check(lib.ccm_optimize_sim3(ctx.handle, C.byref(pb)))
        t3 = time.perf_counter()
        t_search.append(t1 - t0); t_list.append(t2 - t1); t_opt.append(t3 - t2)
        pruned = np.zeros(sum1, np.uint8)
        for k, c in enumerate(corr):
            pruned[f1[k] + c[inl[first[k]:first[k + 1]] == 0, 0]] = 1
        state.update(a_s3=s3, a_nin=nin, a_pruned=pruned, corr=corr, rows=int(first[-1]))

    def route_b():
        t0 = time.perf_counter()
        state["b_total"] = ctx.check(lib.ccm_compute_sim3_table_frames(ctx.handle, C.c_void_p(table.handle), C.byref(cprob), C.byref(rb)))
        t_b.append(time.perf_counter() - t0)

    def same():
        return (state["a_total"] == state["b_total"] and a_m12.tobytes() == b_m12.tobytes() and state["a_s3"].tobytes() == b_s3.tobytes() and
                state["a_nin"].tobytes() == b_nin.tobytes() and state["a_pruned"].tobytes() == b_pruned.tobytes() and
                [len(c) for c in state["corr"]] == b_nc.tolist())

    for _ in range(a.warmup):
        route_a(); route_b()
    assert all(host_list(sc, q, a_m12[f1[k]:f1[k + 1]]).tobytes() == X.correspondences(sc["rows"], sc["capacity"], q, a_m12[f1[k]:f1[k + 1]]).tobytes()
               for k, q in enumerate(pairs))
    for v in (t_search, t_list, t_opt, t_b):
        v.clear()
    mismatches = 0
    for r in range(a.reps):
        if r % 2 == 0:
            route_a(); route_b()
        else:
            route_b(); route_a()
        mismatches += not same()
    rows = state["rows"]
    # host-to-device bytes.  The search's staging copy is common to both routes.  Behind it (a) uploads per problem sim3, fix_scale, K1, K2,
    # first, th2 and 112 bytes a correspondence, and downloads match12 in between; (b) adds per pair the 168-byte view and sim3, K1, K2,
    # fix_scale, th2, and the two level tables
    common = seg(2 * n_pairs * 168) + seg(2 * n_pairs * 80) + seg(n_pairs * 16) + 2 * seg(sum1 * 4)
    a_up = common + n_pairs * (64 + 4 + 32 + 32 + 4) + (n_pairs + 1) * 4 + rows * 112
    b_up = common + seg(n_pairs * 64) + 2 * seg(n_pairs * 32) + 2 * seg(n_pairs * 4) + seg(n_pairs * 168) + 2 * 64
    calls = np.asarray(t_search) + np.asarray(t_opt)
    sa, sb = stats(calls), stats(t_b)
    out = dict(pairs=n_pairs, features=[n1, [len(q["kf2"]["kx"]) for q in pairs]], found=int(state["b_total"]), correspondences=b_nc.tolist(),
               n_inliers=b_nin.tolist(), pruned=int(b_pruned.sum()), mismatching_reps=int(mismatches),
               a_search_call=stats(t_search), a_host_list_numpy=stats(t_list), a_optimize_call=stats(t_opt), a_two_calls=sa, b_chain_call=sb,
               a_upload_bytes=int(a_up), b_upload_bytes=int(b_up), ratio_a_calls_over_b=round(sa["median_ms"] / sb["median_ms"], 3),
               b_faster_outside_spread=bool(sb["p90_ms"] < sa["p10_ms"]))
    print("%d pair(s): (a) search %.3f + list %.3f + optimise %.3f ms, two calls %.3f [%.3f, %.3f] | (b) %.3f [%.3f, %.3f] | a calls / b = %.2f | upload %d -> %d"
          " bytes | correspondences %d | mismatches %d" % (n_pairs, out["a_search_call"]["median_ms"], out["a_host_list_numpy"]["median_ms"],
                                                         out["a_optimize_call"]["median_ms"], sa["median_ms"], sa["p10_ms"], sa["p90_ms"], sb["median_ms"],
                                                         sb["p10_ms"], sb["p90_ms"], out["ratio_a_calls_over_b"], a_up, b_up, rows, mismatches), flush=True)
    for h in hs.values():
        h.close()
    table.close()
    return out, mismatches


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out", default=None, help="output file (default profiles/<tag>_sim3_chain.json)")
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    lib = _lib.load()
    result = {"workload": {"reps": a.reps, "warmup": a.warmup}, "sizes": {}}
    bad = 0
    for n in (1, 3, 8):
        out, b = bench(ctx, lib, n, a)
        result["sizes"]["chain_%d" % n] = out
        bad += int(b)
    path = a.out or os.path.join(ROOT, "profiles", "%s_sim3_chain.json" % a.tag)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: (v["a_two_calls"]["median_ms"], v["b_chain_call"]["median_ms"], v["ratio_a_calls_over_b"], v["b_faster_outside_spread"],
                          v["mismatching_reps"]) for k, v in result["sizes"].items()}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
