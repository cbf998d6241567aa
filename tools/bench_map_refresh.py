"""ComputeDistinctiveDescriptors + UpdateNormalAndDepth for the map points a keyframe insertion or a bundle adjustment touched:
the host route against ccm_map_table_refresh on keyframe handles (include/ccm_hot.h "map-point table").

Two sizes, both with 20 keyframes of 1,000 features:
  local_mapping  about 2,500 points with 8 observations on average, descriptor and normal / depth, positions already in the table
  local_ba       20,000 points, normal / depth only, the new positions given in the call
Routes, alternating inside one process after a warm-up (page-locked staging warmed by it), each timed with the host clock around work
that ends in a synchronisation, the rows of the two tables compared after every repetition:
  (a) the parent's route: gather the observed descriptors on the host, ccm_distinctive_descriptors (upload, kernel, download), normal
      and min / max distance on the host (tests/map_refresh_ref.py normal_depth_batch: numpy vectorised over the points, standing in
      for the reference's per-point loop; timed separately), ccm_map_table_update of the rows, synchronise
  (b) ccm_map_table_refresh with its one download (what the host's MapPoint objects keep)
  (c) ccm_map_table_refresh without a result, then a synchronisation: the device part alone (the call itself returns without waiting)
Output: profiles/<tag>_map_refresh.json and one summary line.

    python tools/bench_map_refresh.py [--reps 30] [--warmup 5] [--tag mi355x]
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

import map_refresh_ref as R  # noqa: E402
from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.frame import DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import FrameGridView  # noqa: E402
from motioncheck_ccm_slam_amd.tracking import MapPointTable  # noqa: E402
from motioncheck_ccm_slam_amd.vocabulary import ORBVocabulary, synthetic_tree  # noqa: E402

COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")
N_KF, N_FEAT = 20, 1000


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def workload(n_points, seed):
    """Keyframes as tests/map_refresh_ref.py's scene makes them (random descriptors), points in the cube in front of them, 2 to 14
    observations each (8 on average) in distinct keyframes, the first one the reference keyframe."""
    rng = np.random.default_rng(seed)
    kfs = []
    for k in range(N_KF):
        Ow = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-4.8, -3.0)], "f4")
        kfs.append(dict(kx=rng.uniform(0, 752, N_FEAT).astype("f4"), ky=rng.uniform(0, 480, N_FEAT).astype("f4"),
                        oct=rng.integers(0, R.N_LEVELS, N_FEAT).astype("i4"), desc=rng.integers(0, 256, (N_FEAT, 32), dtype=np.uint8), Ow=Ow,
                        Tcw=np.concatenate([np.eye(3, dtype="f4"), -Ow[:, None]], 1).astype("f4"), sf=R.SCALE, sigma2=R.SIGMA2))
    counts = rng.integers(2, 15, n_points).astype("i4")
    first = np.concatenate([[0], np.cumsum(counts)]).astype("i4")
    okf = np.concatenate([rng.permutation(N_KF)[:c] for c in counts]).astype("i4")
    ofeat = rng.integers(0, N_FEAT, first[-1]).astype("i4")
    return dict(kfs=kfs, slot=rng.permutation(n_points).astype("i4"), pos=rng.uniform(-0.7, 0.7, (n_points, 3)).astype("f4"), counts=counts,
                obs_first=first, obs_kf=okf, obs_feat=ofeat, ref_kf=okf[first[:-1]].copy(), ref_feat=ofeat[first[:-1]].copy())


def same(a, b):
    for k in COLS:
        x = np.ascontiguousarray(a[k]); y = np.ascontiguousarray(b[k])
        if x.dtype.kind == "f":
            nx, ny = np.isnan(x), np.isnan(y)
            if not ((nx == ny).all() and (x.view("u4")[~nx] == y.view("u4")[~ny]).all()):
                return False
        elif not (x == y).all():
            return False
    return True


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out", default=None, help="output file (default profiles/<tag>_map_refresh.json)")
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    par, vdesc, w = synthetic_tree(3, 2, seed=1, ragged=False)
    voc = ORBVocabulary(3, 2, par, vdesc, w, ctx=ctx)                # ccm_distinctive_descriptors hangs off a vocabulary handle
    result = {"workload": {"keyframes": N_KF, "features": N_FEAT, "reps": a.reps, "warmup": a.warmup}, "sizes": {}}
    bad = 0
    for name, n_points, what, give_pos in (("local_mapping", 2500, 3, False), ("local_ba", 20000, R.NORMAL_DEPTH, True)):
        S = workload(n_points, 7)
        kfs = S["kfs"]
        handles = []
        for kf in kfs:
            h = DeviceFrame(FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"]), None, ctx=ctx)
            h.set_camera(np.array(R.INTR, "f4"), kf["sf"], kf["sigma2"]); h.set_pose(kf["Tcw"], kf["Ow"])
            handles.append(h)
        rows = R.table_rows(3, n_points)
        if not give_pos:
            rows["pos"][S["slot"]] = S["pos"]
        ta, tb = MapPointTable(n_points, ctx=ctx), MapPointTable(n_points, ctx=ctx)
        Ow_kf = np.stack([k["Ow"] for k in kfs])
        lvl = np.array([kfs[k]["oct"][f] for k, f in zip(S["ref_kf"], S["ref_feat"])])
        stacked = R.stacked_descriptors(S)                          # the keyframes' own descriptor arrays, there before the call
        t_gather, t_dd, t_host, t_upd, t_b, t_c = [], [], [], [], [], []

        def reset():
            for t in (ta, tb):
                t.update(np.arange(n_points), **{k: rows[k] for k in COLS})
            ctx.sync()

        def route_a():
            t0 = time.perf_counter()
            cols = {}
            if what & R.DESCRIPTOR:
                g, first, count = R.gathered_descriptors(S, stacked)
                t1 = time.perf_counter()
                best = voc.distinctive_descriptors(g, first, count)
                cols["desc"] = g[first + best]
                t2 = time.perf_counter()
            else:
                t1 = t2 = t0
            nrm, mn, mx = R.normal_depth_batch(S["pos"], Ow_kf, S["obs_first"], S["obs_kf"], Ow_kf[S["ref_kf"]], R.SCALE[lvl],
                                               np.full(n_points, R.SCALE[-1]))
            t3 = time.perf_counter()
            if give_pos:
                cols["pos"] = S["pos"]
            ta.update(S["slot"], normal=nrm, min_dist=mn, max_dist=mx, **cols)
            ctx.sync()
            t4 = time.perf_counter()
            t_gather.append(t1 - t0); t_dd.append(t2 - t1); t_host.append(t3 - t2); t_upd.append(t4 - t3)

        def route_b(fetch=True):
            t0 = time.perf_counter()
            tb.refresh(S["slot"], handles, S["obs_first"], S["obs_kf"], S["obs_feat"], S["ref_kf"], S["ref_feat"],
                       pos=S["pos"] if give_pos else None, what=what, fetch=fetch)
            if not fetch:
                ctx.sync()
            (t_b if fetch else t_c).append(time.perf_counter() - t0)

        for _ in range(a.warmup):
            reset(); route_a(); route_b(); route_b(False)
        for v in (t_gather, t_dd, t_host, t_upd, t_b, t_c):
            v.clear()
        mismatches = 0
        for r in range(a.reps):
            reset()
            if r % 2 == 0:
                route_a(); route_b()
            else:
                route_b(); route_a()
            all_slots = np.arange(n_points)
            mismatches += not same(ta.fetch(all_slots), tb.fetch(all_slots))
            reset(); route_b(False)
        total_a = np.array(t_gather) + np.array(t_dd) + np.array(t_host) + np.array(t_upd)
        n_obs = int(S["obs_first"][-1])
        res = {"points": n_points, "observations": n_obs, "what": int(what), "pos_in_call": give_pos, "mismatching_reps": int(mismatches),
               "a_gather_host": stats(t_gather), "a_distinctive_descriptors": stats(t_dd), "a_normal_depth_host": stats(t_host),
               "a_table_update_sync": stats(t_upd), "a_total": stats(total_a), "b_refresh_with_download": stats(t_b),
               "c_refresh_no_result_then_sync": stats(t_c),
               "a_upload_bytes": (32 * n_obs + 12 * n_points if what & R.DESCRIPTOR else 0) + n_points * (4 + 20 + (32 if what & R.DESCRIPTOR else 0) + (12 if give_pos else 0)),
               "b_upload_bytes": n_points * (4 + 4 + (8 if what & R.NORMAL_DEPTH else 0) + (12 if give_pos else 0)) + 8 * n_obs + 40 * N_KF}
        res["ratio_a_over_b"] = round(res["a_total"]["median_ms"] / res["b_refresh_with_download"]["median_ms"], 3)
        result["sizes"][name] = res
        bad += mismatches
        print("%-13s %6d points %7d obs | (a) gather %.3f + distinctive %.3f + host normal %.3f + update %.3f = %.3f ms | (b) refresh %.3f ms |"
              " (c) no result + sync %.3f ms | a / b = %.2f | mismatches %d" % (
                  name, n_points, n_obs, res["a_gather_host"]["median_ms"], res["a_distinctive_descriptors"]["median_ms"],
                  res["a_normal_depth_host"]["median_ms"], res["a_table_update_sync"]["median_ms"], res["a_total"]["median_ms"],
                  res["b_refresh_with_download"]["median_ms"], res["c_refresh_no_result_then_sync"]["median_ms"], res["ratio_a_over_b"], mismatches),
              flush=True)
        for h in handles:
            h.close()
        ta.close(); tb.close()
    out = a.out or os.path.join(ROOT, "profiles", "%s_map_refresh.json" % a.tag)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: (v["a_total"]["median_ms"], v["b_refresh_with_download"]["median_ms"], v["ratio_a_over_b"], v["mismatching_reps"])
                      for k, v in result["sizes"].items()}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
