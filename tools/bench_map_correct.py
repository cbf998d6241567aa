"""The keyframe and map-point correction of a loop closure or a map merge: the array route against ccm_map_table_correct_frames on
keyframe handles and the map-point table (include/ccm_hot.h "loop and merge corrections on the table").

Two shapes, keyframes of 1,000 features, about 5 observations per point, every point owned by a moved keyframe, poses first (the
order in which the two routes compute the same thing):
  loop    30 moved keyframes and 10 that are only observed, 8,000 points
  merge   500 moved keyframes, 100,000 points
Routes, alternating inside one process after a warm-up (page-locked staging warmed by it), each timed with the host clock around work
that ends in a synchronisation; the rows of the two tables and the poses of the two sets of handles are compared bit for bit after
every repetition:
  (a) today's route: Optimizer.CorrectMapPoints on float64 arrays (upload, kernel, download), table.update(pos), one set_pose per
      moved keyframe, table.refresh(NORMAL_DEPTH) with its download; each step timed
  (b) MapPointTable.correct with its one download (what the host's MapPoint objects keep)
  (c) MapPointTable.correct without outputs, then a synchronisation: the device part alone (the call itself returns without waiting)
The new poses of route (a) are computed before the clock starts, as the Sim3 arrays of route (b) are.
Output: profiles/<tag>_map_correct.json and one summary line.

    python tools/bench_map_correct.py [--reps 20] [--warmup 3] [--tag mi355x]
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

import map_correct_ref as MC  # noqa: E402
import map_refresh_ref as R  # noqa: E402
from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.frame import DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import FrameGridView  # noqa: E402
from motioncheck_ccm_slam_amd.optimizer import Optimizer  # noqa: E402
from motioncheck_ccm_slam_amd.tracking import MapPointTable  # noqa: E402
from optimizer_cases import quat_R, rand_sim3  # noqa: E402

COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")
N_FEAT = 1000
MAP_CAM_BYTES, REFRESH_VIEW_BYTES, CORRECT_VIEW_BYTES = 96, 40, 32      # sizeof MapCam, MptKfView, MptCorrectKf (csrc)


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def workload(n_moved, n_still, n_points, seed):
    """Keyframes in a slab in front of the cloud (as tests/map_refresh_ref.py's scene), points in the cube, 2 to 8 observations each
    (5 on average) in distinct keyframes, the first one the reference keyframe; a Sim3 pair per moved keyframe as
    tests/map_correct_ref.py's scene makes them."""
    rng = np.random.default_rng(seed)
    n_kf = n_moved + n_still
    kfs = []
    for k in range(n_kf):
        Ow = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-4.8, -3.0)], "f4")
        kfs.append(dict(kx=rng.uniform(0, 752, N_FEAT).astype("f4"), ky=rng.uniform(0, 480, N_FEAT).astype("f4"),
                        oct=rng.integers(0, R.N_LEVELS, N_FEAT).astype("i4"), desc=rng.integers(0, 256, (N_FEAT, 32), dtype=np.uint8), Ow=Ow,
                        Tcw=np.concatenate([np.eye(3, dtype="f4"), -Ow[:, None]], 1).astype("f4"), sf=R.SCALE, sigma2=R.SIGMA2))
    counts = rng.integers(2, 9, n_points).astype("i4")
    first = np.concatenate([[0], np.cumsum(counts)]).astype("i4")
    okf = (rng.integers(0, n_kf, n_points)[:, None] + np.arange(8)[None, :] * 7) % n_kf       # distinct for 40 and for 500 keyframes
    okf = np.concatenate([okf[p, :c] for p, c in enumerate(counts)]).astype("i4")
    ofeat = rng.integers(0, N_FEAT, first[-1]).astype("i4")
    before = np.zeros((n_moved, 8)); after = np.zeros((n_moved, 8))
    for k in range(n_moved):
        Ow = kfs[k]["Ow"].astype("f8")
        before[k] = [0, 0, 0, 1, -Ow[0], -Ow[1], -Ow[2], 1]
        d = rand_sim3(rng)
        after[k, :4] = d[:4]; after[k, 7] = d[7]
        after[k, 4:7] = -d[7] * (quat_R(d[:4]) @ (Ow + rng.uniform(-0.5, 0.5, 3)))
    return dict(kfs=kfs, n_moved=n_moved, slot=rng.permutation(n_points).astype("i4"), pos=rng.uniform(-0.7, 0.7, (n_points, 3)).astype("f4"),
                owner=rng.integers(0, n_moved, n_points).astype("i4"), obs_first=first, obs_kf=okf, obs_feat=ofeat,
                ref_kf=okf[first[:-1]].copy(), ref_feat=ofeat[first[:-1]].copy(), sim3_before=before, sim3_after=after)


def same_rows(a, b):
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out", default=None, help="output file (default profiles/<tag>_map_correct.json)")
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    result = {"workload": {"features": N_FEAT, "reps": a.reps, "warmup": a.warmup, "order": "poses_first", "transform": "sim3"}, "shapes": {}}
    bad = 0
    for name, n_moved, n_still, n_points in (("loop", 30, 10, 8000), ("merge", 500, 0, 100000)):
        S = workload(n_moved, n_still, n_points, 11)
        kfs = S["kfs"]; n_kf = len(kfs)

        def make_handles():
            hs = []
            for kf in kfs:
                h = DeviceFrame(FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"]), None, ctx=ctx)
                h.set_camera(np.array(R.INTR, "f4"), kf["sf"], kf["sigma2"]); h.set_pose(kf["Tcw"], kf["Ow"])
                hs.append(h)
            return hs
        ha, hb = make_handles(), make_handles()
        rows = R.table_rows(3, n_points)
        rows["pos"][S["slot"]] = S["pos"]
        ta, tb = MapPointTable(n_points, ctx=ctx), MapPointTable(n_points, ctx=ctx)
        new_poses = [MC.new_pose(s) for s in S["sim3_after"]]
        pos64 = S["pos"].astype("f8")
        lists = (S["obs_first"], S["obs_kf"], S["obs_feat"], S["ref_kf"], S["ref_feat"])
        t_arr, t_upd, t_pose, t_ref, t_b, t_c = [], [], [], [], [], []

        def reset():
            for t in (ta, tb):
                t.update(np.arange(n_points), **{k: rows[k] for k in COLS})
            for hs in (ha, hb):
                for h, kf in zip(hs[:n_moved], kfs):
                    h.set_pose(kf["Tcw"], kf["Ow"])
            ctx.sync()

        def route_a():
            t0 = time.perf_counter()
            new = Optimizer.CorrectMapPoints(pos64, S["owner"], S["sim3_before"], S["sim3_after"], ctx=ctx).astype("f4")
            t1 = time.perf_counter()
            ta.update(S["slot"], pos=new)
            t2 = time.perf_counter()
            for h, (T, O) in zip(ha, new_poses):
                h.set_pose(T, O)
            t3 = time.perf_counter()
            ta.refresh(S["slot"], ha, *lists, what=R.NORMAL_DEPTH)
            t4 = time.perf_counter()
            t_arr.append(t1 - t0); t_upd.append(t2 - t1); t_pose.append(t3 - t2); t_ref.append(t4 - t3)

        def route_b(fetch=True):
            t0 = time.perf_counter()
            tb.correct(hb, n_moved, S["slot"], S["owner"], sim3_before=S["sim3_before"], sim3_after=S["sim3_after"], lists=lists, fetch=fetch)
            if not fetch:
                ctx.sync()
            (t_b if fetch else t_c).append(time.perf_counter() - t0)

        for _ in range(a.warmup):
            reset(); route_a(); route_b(); reset(); route_b(False)
        for v in (t_arr, t_upd, t_pose, t_ref, t_b, t_c):
            v.clear()
        mismatches = 0
        all_slots = np.arange(n_points)
        for r in range(a.reps):
            reset()
            if r % 2 == 0:
                route_a(); route_b()
            else:
                route_b(); route_a()
            ok = same_rows(ta.fetch(all_slots), tb.fetch(all_slots))
            for x, y in zip(ha, hb):
                (Tx, Ox), (Ty, Oy) = x.pose(), y.pose()
                ok = ok and Tx.tobytes() == Ty.tobytes() and Ox.tobytes() == Oy.tobytes()
            mismatches += not ok
            reset(); route_b(False)
        total_a = np.array(t_arr) + np.array(t_upd) + np.array(t_pose) + np.array(t_ref)
        n_obs = int(S["obs_first"][-1]); n = n_points
        lists_bytes = 4 * (n + 1) + 8 * n_obs + 8 * n
        res = {"keyframes": n_kf, "moved": n_moved, "points": n, "observations": n_obs, "mismatching_reps": int(mismatches),
               "a_correct_map_points": stats(t_arr), "a_table_update": stats(t_upd), "a_set_pose_per_keyframe": stats(t_pose),
               "a_refresh_with_download": stats(t_ref), "a_total": stats(total_a), "b_correct_with_download": stats(t_b),
               "c_correct_no_outputs_then_sync": stats(t_c),
               "a_upload_bytes": 28 * n + 128 * n_moved + 16 * n + MAP_CAM_BYTES * n_moved + 4 * n + lists_bytes + REFRESH_VIEW_BYTES * n_kf,
               "a_download_bytes": 24 * n + 24 * n, "a_calls": 3 + n_moved,
               "b_upload_bytes": 8 * n + lists_bytes + 128 * n_moved + CORRECT_VIEW_BYTES * n_kf, "b_download_bytes": 32 * n, "b_calls": 1}
        res["ratio_a_over_b"] = round(res["a_total"]["median_ms"] / res["b_correct_with_download"]["median_ms"], 3)
        result["shapes"][name] = res
        bad += mismatches
        print("%-6s %4d kf %6d points %7d obs | (a) arrays %.3f + update %.3f + set_pose %.3f + refresh %.3f = %.3f ms | (b) correct %.3f ms |"
              " (c) no outputs + sync %.3f ms | a / b = %.2f | mismatches %d" % (
                  name, n_kf, n, n_obs, res["a_correct_map_points"]["median_ms"], res["a_table_update"]["median_ms"],
                  res["a_set_pose_per_keyframe"]["median_ms"], res["a_refresh_with_download"]["median_ms"], res["a_total"]["median_ms"],
                  res["b_correct_with_download"]["median_ms"], res["c_correct_no_outputs_then_sync"]["median_ms"], res["ratio_a_over_b"], mismatches),
              flush=True)
        for h in ha + hb:
            h.close()
        ta.close(); tb.close()
    out = a.out or os.path.join(ROOT, "profiles", "%s_map_correct.json" % a.tag)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: (v["a_total"]["median_ms"], v["b_correct_with_download"]["median_ms"], v["ratio_a_over_b"], v["mismatching_reps"])
                      for k, v in result["shapes"].items()}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
