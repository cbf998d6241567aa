#!/usr/bin/env python3
"""Times ccm_covis_query on a server-sized synthetic map: --keyframes (2000) keyframes of --features (2000) features, of which
--with-point (600) hold a map point; the points lie along the trajectory so that each is seen by about six keyframes and a keyframe
shares points with about forty neighbours; a map-point table of --table (200 000) slots, one row in a hundred BAD.

  call       host clock around ccm_covis_query (it synchronises before it returns): median [p10, p90] of --reps steady-state
             queries (nothing pending) after --warmup, for n_q = 1, 64 and 500 keyframes per query, weights only and weights plus
             redundancy
  flush / kernel / download
             HIP events inside the same calls (ccm_covis_last_timing), medians
  first      the one query that uploads the whole map (every put pending)
  put        a replaced record followed by a query of it: what UpdateConnections of one changed keyframe costs
  culling    mapping.KeyFrameCulling over 100 consecutive local keyframes (culled records are put back between repetitions)
  numpy      for context, the same counts for ONE keyframe from the observation lists (point -> keyframes) with numpy on one core:
             the gather the reference's walk does with std::map copies.  It is not the reference.

Output: profiles/covisibility.json and a summary line per shape.  Needs the GPU; nothing here runs on a CPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

try:
    import torch  # noqa: F401  (first, so that the library binds to the same HIP runtime as in the tests)
except ImportError:
    pass

from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.covisibility import COVIS_REDUNDANCY, COVIS_WEIGHTS, CovisibilityIndex  # noqa: E402
from motioncheck_ccm_slam_amd.mapping import KeyFrameCulling  # noqa: E402
from motioncheck_ccm_slam_amd.tracking import MapPointTable  # noqa: E402


def stats(ms):
    t = np.asarray(ms, "f8")
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def synthetic_map(a, rng):
    """records: per keyframe (slot [features], octave [features]); a point p is seen from a window of keyframes around p"""
    step = a.table / a.keyframes                                        # points the trajectory advances per keyframe
    window = int(step * 20)
    records = []
    for k in range(a.keyframes):
        lo = int(k * step) - window // 2
        pts = (lo + rng.choice(window, a.with_point, replace=False)) % a.table
        slot = np.full(a.features, -1, "i4")
        slot[rng.choice(a.features, a.with_point, replace=False)] = pts
        records.append((slot, rng.choice(8, a.features, p=[.3, .2, .15, .1, .1, .05, .05, .05]).astype(np.uint8)))
    return records


def numpy_walk(records, flags, n_keys, rng):
    """One core, numpy: KFcounter and the culling counts of one keyframe from the observation lists."""
    kf = np.concatenate([np.full(len(s), k, "i4") for k, (s, _) in enumerate(records)])
    slot = np.concatenate([s for s, _ in records]); octave = np.concatenate([o for _, o in records])
    keep = slot >= 0
    kf, slot, octave = kf[keep], slot[keep], octave[keep]
    order = np.argsort(slot, kind="stable")
    kf, slot, octave = kf[order], slot[order], octave[order]
    first = np.searchsorted(slot, np.arange(len(flags) + 1))            # observations of point p: first[p] .. first[p + 1]
    t_w, t_r = [], []
    for k in rng.integers(0, len(records), n_keys):
        s, o = records[k]
        t0 = time.perf_counter()
        mine = s[s >= 0]; mine_o = o[s >= 0]
        ok = (flags[mine] & 3) == 1
        mine, mine_o = mine[ok], mine_o[ok]
        n_obs = first[mine + 1] - first[mine]
        idx = np.repeat(first[mine], n_obs) + (np.arange(n_obs.sum()) - np.repeat(np.cumsum(n_obs) - n_obs, n_obs))
        others = kf[idx] != k
        weights = np.bincount(kf[idx][others], minlength=len(records))
        t1 = time.perf_counter()
        fine = others & (octave[idx] <= np.repeat(mine_o, n_obs).astype("i4") + 1)
        per_point = np.add.reduceat(fine, np.cumsum(n_obs) - n_obs) if len(mine) else np.zeros(0, "i8")
        n_red = int((per_point >= 3).sum())
        t2 = time.perf_counter()
        t_w.append((t1 - t0) * 1e3); t_r.append((t2 - t0) * 1e3)
        assert weights[k] == 0 and n_red >= 0
    return stats(t_w), stats(t_r)


def timed_queries(ix, table, keys_of, what, a):
    for i in range(a.warmup):
        ix.query(keys_of(i), table=table, what=what)
    call, parts = [], []
    for i in range(a.reps):
        keys = keys_of(a.warmup + i)
        t0 = time.perf_counter()
        ix.query(keys, table=table, what=what)
        call.append((time.perf_counter() - t0) * 1e3)
        parts.append(ix.last_timing())
    parts = np.asarray(parts)
    return {"call": stats(call), "flush": stats(parts[:, 0]), "kernel": stats(parts[:, 1]), "download": stats(parts[:, 2])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--with-point", type=int, default=600)
    ap.add_argument("--table", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covisibility.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    ctx = _lib.Context(0)                                              # raises without a GPU: there is no CPU path to time
    records = synthetic_map(a, rng)
    flags = np.full(a.table, _lib.MP_LIVE, np.uint8)
    flags[rng.choice(a.table, a.table // 100, replace=False)] |= _lib.MP_BAD
    table = MapPointTable(a.table, ctx=ctx)
    table.update(np.arange(a.table, dtype="i4"), flags=flags)
    ix = CovisibilityIndex(1 << 20, ctx=ctx)                           # smaller than the data: the first flush also grows the arena
    t0 = time.perf_counter()
    for k, (s, o) in enumerate(records):
        ix.put(k, s, o)
    t_put = time.perf_counter() - t0
    t0 = time.perf_counter()
    r = ix.query([0], table=table)
    first_ms = (time.perf_counter() - t0) * 1e3
    first = ix.last_timing()
    cap, used, live = ix.arena()
    res = {"device": "MI355X", "keyframes": a.keyframes, "features": a.features, "features_with_point": a.with_point, "table_slots": a.table,
           "lds_features": ix.lds_features(), "arena_features": live, "arena_bytes": live * 5, "put_us_per_keyframe": round(t_put / a.keyframes * 1e6, 2),
           "first_query": {"call_ms": round(first_ms, 3), "flush_ms": round(first[0], 3), "kernel_ms": round(first[1], 4), "download_ms": round(first[2], 4)},
           "queries": []}
    full = ix.query(list(range(0, a.keyframes, max(a.keyframes // 50, 1))), table=table)
    res["observers_per_point"] = round(float(full.weights.sum()) / max(float(full.n_mps.sum()), 1) + 1, 2)
    res["neighbours_per_keyframe"] = round(float((full.weights > 0).sum()) / len(full.weights), 1)
    res["redundant_share"] = round(float(full.n_redundant.sum()) / max(float(full.n_mps.sum()), 1), 3)
    for n_q in (1, 64, 500):
        n_q = min(n_q, a.keyframes)
        keys_of = lambda i, n_q=n_q: [(37 * i + 3 * j) % a.keyframes for j in range(n_q)]     # noqa: E731
        for what, name in ((COVIS_WEIGHTS, "weights"), (COVIS_WEIGHTS | COVIS_REDUNDANCY, "weights+redundancy")):
            q = timed_queries(ix, table, keys_of, what, a)
            q.update({"n_q": n_q, "what": name})
            res["queries"].append(q)
            print("covis n_q %3d %-18s: call %.3f ms [%.3f, %.3f] = flush %.4f + kernel %.4f + download %.4f" %
                  (n_q, name, q["call"]["median_ms"], q["call"]["p10_ms"], q["call"]["p90_ms"], q["flush"]["median_ms"],
                   q["kernel"]["median_ms"], q["download"]["median_ms"]))
    # one changed keyframe: put, then its weights
    t_upd = []
    for i in range(a.reps):
        k = (91 * i) % a.keyframes
        t0 = time.perf_counter()
        ix.put(k, *records[k])
        ix.query([k], table=table, what=COVIS_WEIGHTS)
        t_upd.append((time.perf_counter() - t0) * 1e3)
    res["put_and_query_one"] = stats(t_upd)
    # the culling driver over 100 consecutive local keyframes
    t_cull, n_culled, n_queries = [], [], []
    for i in range(max(a.reps // 10, 3)):
        lo = (173 * i) % max(a.keyframes - 100, 1)
        local = list(range(lo, min(lo + 100, a.keyframes)))
        calls = [0]
        real_query = ix.query

        def counting_query(*args, **kw):
            calls[0] += 1
            return real_query(*args, **kw)
        ix.query = counting_query
        t0 = time.perf_counter()
        culled = KeyFrameCulling(ix, table, local, local[:2], 0.9)
        t_cull.append((time.perf_counter() - t0) * 1e3)
        del ix.query
        n_culled.append(len(culled)); n_queries.append(calls[0])
        for k in culled:
            ix.put(k, *records[k])
        ix.query([0], table=table, what=COVIS_WEIGHTS)                  # (the flush of the records put back is not the driver's)
    res["culling_100_local"] = dict(stats(t_cull), culled_median=float(np.median(n_culled)), queries_median=float(np.median(n_queries)))
    w, rd = numpy_walk(records, flags, 30, rng)
    res["numpy_one_core_per_keyframe"] = {"weights": w, "weights+redundancy": rd}
    print("covis put+query of one keyframe %.3f ms; culling over 100 local keyframes %.3f ms (%g culled, %g queries); "
          "numpy on one core, per keyframe: weights %.3f ms, with redundancy %.3f ms; first query %.1f ms; arena %.1f MB" %
          (res["put_and_query_one"]["median_ms"], res["culling_100_local"]["median_ms"], res["culling_100_local"]["culled_median"],
           res["culling_100_local"]["queries_median"], w["median_ms"], rd["median_ms"], first_ms, live * 5 / 1e6))
    table.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
