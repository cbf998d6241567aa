"""Tracking::TrackWithMotionModel behind the pose product: ccm_frame_track_motion_model against the route it replaces.

Workload: two extractions of a synthetic 752x480 image (the second moved by (-5, +3) pixels) at 1000 and 2000 requested features, the
last frame's features as map points in a table (tests/track_motion_model_ref.py, matchable_scene).  Per tracked frame, timed with the
host clock around calls that end in a stream synchronisation, the two routes alternating in one process after a warm-up:
  old  four calls on a pair of handles: ccm_frame_set_map_points (clear) -> ccm_frame_search_by_projection_frame (valid, u, v,
       descriptors and flags of every last-frame feature uploaded; the projection itself is made before the clock starts, so the
       old route is charged less than it costs) -> ccm_frame_pose_optimize_table -> ccm_frame_set_map_points (outliers dropped)
  new  one ccm_frame_track_motion_model on a second pair of handles
Every repetition's match, pose7, outlier and mp_id are compared between the routes.  The uploaded bytes are computed from the two
staging layouts (csrc/frame_window_host.cpp frame_window, frame_pose_host.cpp frame_pose_run, frame_host.cpp ccm_frame_set_map_points; csrc/mpt_track_host.cpp).
Output: profiles/<tag>_track_motion_model.json and one summary line.

    python tools/bench_track_motion_model.py [--reps 200] [--warmup 20] [--tag r05]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import search_local_points_ref as R  # noqa: E402
import track_motion_model_ref as M  # noqa: E402
from motioncheck_ccm_slam_amd import _lib, synth  # noqa: E402
from motioncheck_ccm_slam_amd.frame import DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import ORBmatcher  # noqa: E402
from motioncheck_ccm_slam_amd.orb import ORBextractor  # noqa: E402
from motioncheck_ccm_slam_amd.tracking import MapPointTable, Tracking  # noqa: E402

INTR = np.array(R.INTR, "f8")
COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")


def seg(n):
    return (n + 63) & ~63


def upload_bytes(n_cur, n_last, n_levels):
    """(old, new) bytes copied host -> device per tracked frame of one search pass, 64-byte segments as the staging areas lay them out."""
    window = seg(4 * n_cur) + seg(n_cur) + 2 * seg(4 * n_last) + 3 * seg(0) + seg(32 * n_last) + 2 * seg(n_last) + seg(4 * n_levels)
    pose = seg(56) + seg(32) + seg(4 * n_levels)
    set_ids = 4 * n_cur                            # the second set_map_points; the first is a device memset
    return window + pose + set_ids, 5 * 64


def pose7_of(Tcw):
    T16 = np.concatenate([np.asarray(Tcw, "f4").reshape(3, 4), np.array([[0, 0, 0, 1]], "f4")]).copy()
    p7 = np.zeros(7)
    assert _lib.load().ccm_pose_from_mat4f(_lib.ptr(T16), _lib.ptr(p7)) == 0
    p7[4:] += [0.02, -0.01, 0.03]
    return p7


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p95_ms": round(float(np.percentile(t, 95)), 4), "n": len(t)}


def run_size(ctx, nfeat, reps, warmup):
    ex = ORBextractor(nfeat, 1.2, 8, 20, 7, ctx=ctx)
    img = synth.frame(7)
    k1, d1 = ex(img); k1, d1 = k1.copy(), d1.copy()
    k2, d2 = ex(np.roll(img, (3, -5), axis=(0, 1)))
    S = M.matchable_scene(k1, d1, k2.copy(), d2.copy(), ex.GetScaleFactors(), ex.GetInverseScaleSigmaSquares())
    rows, Tcw = S["rows"], S["cam"]
    cap = len(rows["flags"])
    q = M.queries(S["last_ids"], rows, Tcw)                                    # the old route's host projection, outside the clock
    pose = pose7_of(Tcw)
    m = ORBmatcher(0.9, True, ctx=ctx)
    t = MapPointTable(cap, ctx=ctx)
    t.update(np.arange(cap), **{k: rows[k] for k in COLS})
    hs = [DeviceFrame(S["last"], S["last_angle"], ctx=ctx), DeviceFrame(S["cur"], S["cur_angle"], ctx=ctx),
          DeviceFrame(S["last"], S["last_angle"], ctx=ctx), DeviceFrame(S["cur"], S["cur_angle"], ctx=ctx)]
    ol, oc, nl, nc = hs
    ol.map_points = S["last_ids"]; nl.map_points = S["last_ids"]
    occ = np.zeros(oc.n, bool)

    def old():
        passes = 0
        for k in (1, 2):
            oc.map_points = None
            nm, match, _ = m.SearchByProjectionFrameHandle(oc, ol, S["scale"], q["valid"], q["u"], q["v"], q["desc"], q["has_obs"], occ, 7.0 * k)
            passes = k
            if nm >= 20:
                break
        if nm < 20:
            return nm, passes, match, None, None, None
        p7, outl, _ = Tracking.PoseOptimizationTable(oc, t, pose, INTR, S["inv_sigma2"])
        ids = np.where(match >= 0, S["last_ids"][np.maximum(match, 0)], -1).astype("i4")
        ids[outl != 0] = -1
        oc.map_points = ids
        ctx.sync()                                                             # set_map_points only queues its copy
        return nm, passes, match, p7, outl, ids

    def new():
        r = Tracking.TrackWithMotionModel(nc, nl, t, Tcw, pose, INTR, S["scale"], S["inv_sigma2"])
        return r.n_matches, r.passes, r.match, r.pose7 if r.posed else None, r.outlier if r.posed else None, r.mp_id if r.posed else None

    def same(a, b):
        return all((x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))

    for _ in range(warmup):
        old(); new()
    t_old, t_new, mismatches = [], [], 0
    for r in range(reps):
        res = {}
        for which in (("old", "new") if r % 2 == 0 else ("new", "old")):       # alternate which route goes first
            f = old if which == "old" else new
            t0 = time.perf_counter(); res[which] = f(); t1 = time.perf_counter()
            (t_old if which == "old" else t_new).append(t1 - t0)
        mismatches += not same(res["old"], res["new"])
    b_old, b_new = upload_bytes(oc.n, ol.n, len(S["scale"]))
    out = {"features_last": ol.n, "features_cur": oc.n, "table_slots": cap, "n_matches": int(res["new"][0]), "passes": int(res["new"][1]),
           "old_route": dict(stats(t_old), upload_bytes=b_old, calls=4), "new_call": dict(stats(t_new), upload_bytes=b_new, calls=1),
           "mismatching_reps": mismatches}
    for h in hs:
        h.close()
    t.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 2000])
    ap.add_argument("--tag", default="r05")
    ap.add_argument("--out", default=None, help="output file (default profiles/<tag>_track_motion_model.json)")
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    result = {"workload": {"image": [752, 480], "reps": a.reps, "warmup": a.warmup, "timed": "host wall clock per tracked frame, synchronised"},
              "sizes": {}}
    for nfeat in a.sizes:
        s = run_size(ctx, nfeat, a.reps, a.warmup)
        result["sizes"][str(nfeat)] = s
        print("%d features requested (%d / %d extracted): old %.4f ms (p95 %.4f, %d bytes up)   new %.4f ms (p95 %.4f, %d bytes up)   "
              "%d matches in %d pass(es), mismatches %d" % (nfeat, s["features_last"], s["features_cur"], s["old_route"]["median_ms"],
              s["old_route"]["p95_ms"], s["old_route"]["upload_bytes"], s["new_call"]["median_ms"], s["new_call"]["p95_ms"],
              s["new_call"]["upload_bytes"], s["n_matches"], s["passes"], s["mismatching_reps"]), flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "%s_track_motion_model.json" % a.tag)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: (v["old_route"]["median_ms"], v["new_call"]["median_ms"], v["mismatching_reps"]) for k, v in result["sizes"].items()}))
    return 1 if sum(v["mismatching_reps"] for v in result["sizes"].values()) else 0


if __name__ == "__main__":
    sys.exit(main())
