"""SearchLocalPoints + pose of TrackLocalMap at map size: host-prepared arrays vs the device-resident map-point table
(include/ccm_hot.h "map-point table").

Workload: one extracted 752x480 frame of 1000 features, its features back-projected as map points, plus random points up to a map of
2,000 / 20,000 / 100,000.  The two paths alternate inside one process after a warm-up, each timed with the host clock around
synchronised calls, and their results are compared on every repetition:
  (a) today's way: the per-point arrays of SearchLocalPoints prepared on the host (tests/search_local_points_ref.py, vectorised
      numpy standing in for the reference's per-point loop; timed separately as `prepare`), then ccm_frame_search_by_projection +
      ccm_frame_pose_optimize over the whole map (every array uploaded per call)
  (b) ccm_frame_search_local_points + ccm_frame_pose_optimize_table
Also timed: one ccm_map_table_update of 500 full rows (a keyframe's worth) followed by a synchronisation, and the share of (b)'s
search call spent in the read-back of the in-view count (ccm_frame_search_local_points_timing).
Output: profiles/<tag>_search_local_points.json and one summary line.

    python tools/bench_search_local_points.py [--reps 100] [--warmup 10] [--maps 2000,20000,100000] [--tag slp]

The Python mirror binds the new symbols when it loads the library, so an older library cannot be loaded beside it (CCM_HOT_LIB is
checked against the mirror).  The comparison point "path (a) on the parent commit" is therefore taken by a second run of this file:

    python tools/bench_search_local_points.py --only-a --package-root <checkout of the parent commit, library built> --tag slp_parent

which imports the package (and so the library) from that checkout, runs path (a) alone on the same workload and writes the same
`a_*` fields.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arg(name, default=None):
    """The value of a `--name VALUE` / `--name=VALUE` option that decides what is imported below."""
    for i, v in enumerate(sys.argv):
        if v == name and i + 1 < len(sys.argv):
            return sys.argv[i + 1]
        if v.startswith(name + "="):
            return v.split("=", 1)[1]
    return default


ONLY_A = "--only-a" in sys.argv
PKG_ROOT = os.path.abspath(_arg("--package-root", ROOT))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, PKG_ROOT)

import numpy as np  # noqa: E402

import search_local_points_ref as R  # noqa: E402
from motioncheck_ccm_slam_amd import _lib, synth  # noqa: E402
from motioncheck_ccm_slam_amd.frame import DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher  # noqa: E402
from motioncheck_ccm_slam_amd.optimizer import Optimizer  # noqa: E402
from motioncheck_ccm_slam_amd.orb import ORBextractor  # noqa: E402
if not ONLY_A:
    from motioncheck_ccm_slam_amd.tracking import MapPointTable, Tracking  # noqa: E402

COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")
CAM = R.camera()
INTR = np.array(R.INTR, "f8")


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def pose7(Tcw):
    T16 = np.concatenate([np.asarray(Tcw, "f4").reshape(3, 4), np.array([[0, 0, 0, 1]], "f4")]).copy()
    p7 = np.zeros(7)
    assert _lib.load().ccm_pose_from_mat4f(_lib.ptr(T16), _lib.ptr(p7)) == 0
    return p7


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--maps", default="2000,20000,100000")
    ap.add_argument("--tag", default="slp")
    ap.add_argument("--out", default=None, help="output file (default profiles/<tag>_search_local_points.json)")
    ap.add_argument("--only-a", action="store_true", help="run path (a) alone (for a library without the map-point table)")
    ap.add_argument("--package-root", default=ROOT, help="import motioncheck_ccm_slam_amd, and its library, from this checkout")
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    lib = _lib.load()
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    kps, desc = ex(synth.frame(1))
    sf, is2 = ex.GetScaleFactors(), ex.GetInverseScaleSigmaSquares()
    fr = FrameGridView(kps["x"], kps["y"], kps["octave"], desc)
    n = len(kps)
    m = ORBmatcher(0.8, ctx=ctx)
    pose0 = pose7(CAM[0]); pose0[4:] += [0.02, -0.01, 0.03]
    result = {"workload": {"image": [752, 480], "features": n, "reps": a.reps, "warmup": a.warmup,
                           "paths": "a" if ONLY_A else "a,b"}, "maps": {}}
    bad = 0
    for M in [int(v) for v in a.maps.split(",")]:
        rows = R.concat(R.matchable_points(fr.kx, fr.ky, fr.oct, desc, *CAM, seed=4), R.random_points(max(M - n, 0), 2))
        cap = len(rows["flags"])
        ids0 = np.where(np.random.default_rng(6).random(n) < 0.3, np.arange(n), -1).astype("i4")   # what the motion model left
        xyz = rows["pos"].astype("f8")
        has_obs = (rows["flags"] & R.HAS_OBS) != 0
        ha = DeviceFrame(fr, kps["angle"], ctx=ctx)
        if not ONLY_A:
            table = MapPointTable(cap, ctx=ctx)
            table.update(np.arange(cap), **{k: rows[k] for k in COLS})
            hb = DeviceFrame(fr, kps["angle"], ctx=ctx)
        t_prep, t_a_search, t_a_pose, t_b_search, t_b_pose, t_rb = [], [], [], [], [], []

        def path_a():
            ha.map_points = ids0
            t0 = time.perf_counter()
            ref = R.replay(ids0, rows, None, *CAM)
            iv = ref["in_view_slot"]                                  # per-point fields, as the reference keeps them on its MapPoints
            in_view = np.zeros(cap, bool); in_view[iv] = True
            level = np.zeros(cap, "i4"); level[iv] = ref["level"]
            vc = np.zeros(cap, "f4"); vc[iv] = ref["view_cos"]
            px = np.zeros(cap, "f4"); px[iv] = ref["proj_x"]
            py = np.zeros(cap, "f4"); py[iv] = ref["proj_y"]
            t1 = time.perf_counter()
            ha.map_points = ref["ids"]
            t2 = time.perf_counter()
            nm, match, occ = m.SearchByProjectionHandle(ha, sf, in_view, level, vc, px, py, rows["desc"], has_obs, ref["occupied"], 1.0)
            t3 = time.perf_counter()
            p7, outl, ni = Optimizer.PoseOptimizationFrame(ha, pose0, INTR, xyz, is2)
            t4 = time.perf_counter()
            t_prep.append(t1 - t0); t_a_search.append(t3 - t2); t_a_pose.append(t4 - t3)
            return nm, ha.map_points, occ, p7, outl, ni, ref["in_view_slot"], ref["level"]

        def path_b():
            hb.map_points = ids0
            t0 = time.perf_counter()
            s = Tracking.SearchLocalPoints(hb, table, CAM[0], R.INTR, sf, Ow=CAM[1], log_scale_factor=R.LOG_SF, taps=True)
            t1 = time.perf_counter()
            p7, outl, ni = Tracking.PoseOptimizationTable(hb, table, pose0, INTR, is2)
            t2 = time.perf_counter()
            ms = np.zeros(3)
            ctx.check(lib.ccm_frame_search_local_points_timing(ctx.handle, _lib.ptr(ms)))
            t_b_search.append(t1 - t0); t_b_pose.append(t2 - t1); t_rb.append(ms.copy())
            return s["nmatches"], s["mp_id"], s["occupied"], p7, outl, ni, s["in_view_slot"], s["level"]

        def a_stats():
            return {"a_prepare_host": stats(t_prep), "a_search_by_projection": stats(t_a_search), "a_pose": stats(t_a_pose),
                    "a_total": stats(np.array(t_prep) + np.array(t_a_search) + np.array(t_a_pose)),
                    "a_upload_bytes_per_frame": cap * (1 + 4 * 4 + 32 + 1 + 3 * 4) + cap * 24}

        if ONLY_A:
            for r in range(a.warmup + a.reps):
                if r == a.warmup:
                    for v in (t_prep, t_a_search, t_a_pose):
                        v.clear()
                ra = path_a()
            res = {"map_points": cap, "in_view": len(ra[6]), "nmatches": int(ra[0]), **a_stats()}
            result["maps"][str(M)] = res
            print("map %6d  in view %5d | (a) prepare %.3f + search %.3f + pose %.3f = %.3f ms" % (
                cap, res["in_view"], res["a_prepare_host"]["median_ms"], res["a_search_by_projection"]["median_ms"],
                res["a_pose"]["median_ms"], res["a_total"]["median_ms"]), flush=True)
            ha.close()
            continue
        for _ in range(a.warmup):
            path_a(); path_b()
        for v in (t_prep, t_a_search, t_a_pose, t_b_search, t_b_pose, t_rb):
            v.clear()
        mismatches = n_view = nm = 0
        for r in range(a.reps):
            ra, rb = (path_a(), path_b()) if r % 2 == 0 else tuple(reversed((path_b(), path_a())))
            n_view, nm = len(rb[6]), int(rb[0])
            mismatches += not all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(ra, rb))
        # a keyframe's worth of rows, synchronised
        t_upd = []
        s500 = np.random.default_rng(3).permutation(cap)[:min(500, cap)]
        upd = {k: rows[k][s500] for k in COLS}
        for r in range(a.warmup + a.reps):
            ctx.sync()
            t0 = time.perf_counter(); table.update(s500, **upd); ctx.sync(); t1 = time.perf_counter()
            if r >= a.warmup:
                t_upd.append(t1 - t0)
        rb = np.array(t_rb)
        res = {"map_points": cap, "in_view": int(n_view), "nmatches": nm, "mismatching_reps": mismatches, **a_stats(),
               "b_search_local_points": stats(t_b_search), "b_pose_table": stats(t_b_pose),
               "b_total": stats(np.array(t_b_search) + np.array(t_b_pose)),
               "b_search_enqueue": stats(rb[:, 0] * 1e-3), "b_search_count_readback": stats(rb[:, 1] * 1e-3),
               "b_search_rest": stats(rb[:, 2] * 1e-3), "table_update_500_rows": stats(t_upd)}
        result["maps"][str(M)] = res
        bad += mismatches
        print("map %6d  in view %5d | (a) prepare %.3f + search %.3f + pose %.3f = %.3f ms | (b) search %.3f (read-back %.3f) + pose %.3f = %.3f ms |"
              " update 500 rows %.3f ms | mismatches %d" % (
                  cap, res["in_view"], res["a_prepare_host"]["median_ms"], res["a_search_by_projection"]["median_ms"], res["a_pose"]["median_ms"],
                  res["a_total"]["median_ms"], res["b_search_local_points"]["median_ms"], res["b_search_count_readback"]["median_ms"],
                  res["b_pose_table"]["median_ms"], res["b_total"]["median_ms"], res["table_update_500_rows"]["median_ms"], mismatches), flush=True)
        ha.close(); hb.close(); table.close()
    out = a.out or os.path.join(ROOT, "profiles", "%s_search_local_points.json" % a.tag)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: (v["a_total"]["median_ms"],) if ONLY_A else (v["a_total"]["median_ms"], v["b_total"]["median_ms"], v["mismatching_reps"])
                      for k, v in result["maps"].items()}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
