"""Per-frame tracking chain: host-buffer entry points vs frame handles (include/ccm_hot.h "frame handles").

Workload: synthetic 752x480 frames, 1000 features, 2000 local map points.  Cases, each timed with the host clock around one
synchronised call, the two paths alternating inside one process after a warm-up:
  (a) SearchByProjection(Frame, map points)         TrackLocalMap (src/Tracking.cpp:905-920)
  (b) SearchByProjection(Current, Last, 7)          TrackWithMotionModel (:571-597)
  (c) PoseOptimizationClient of one frame
  (d) the chain: extract of one frame from host buffers -> frame (handle) -> (b) -> pose -> drop the outliers -> (a) -> pose
  (e) a camera with distortion (the EuRoC one, k1 = -0.2834): extract on the device -> handle -> (b) -> pose, two ways.  Today's
      route: read back the count and the keypoints, Frame::UndistortKeyPoints on the host (ccm_undistort_points), ccm_frame_from_extract
      with the two coordinate arrays.  New route: ccm_frame_from_extract_camera, the undistortion done in the build kernel.
  (f) the handles of 256 images of one extract: 256 calls of ccm_frame_from_extract_camera against one ccm_frames_from_extract_camera
Every repetition's results are compared between the paths.  Output: profiles/<tag>_tracking_chain.json and one summary line.

    python tools/bench_tracking.py [--reps 300] [--warmup 30] [--tag r04]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from motioncheck_ccm_slam_amd import _lib, synth  # noqa: E402
from motioncheck_ccm_slam_amd.frame import Camera, DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher  # noqa: E402
from motioncheck_ccm_slam_amd.optimizer import Optimizer  # noqa: E402
from motioncheck_ccm_slam_amd.orb import ORBextractor  # noqa: E402

INTR = np.array([458.0, 457.0, 367.0, 248.0])
SHIFT = (2, -3)                                   # the current image = the last one moved 2 rows down, 3 columns left


def setup(ctx):
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    last_img = synth.frame(7)
    cur_img = np.roll(last_img, SHIFT, axis=(0, 1))
    kl, dl = ex(last_img)
    kc, dc = ex(cur_img)
    rng = np.random.default_rng(1)
    # the map: the last frame's features back-projected (1000) + points seen elsewhere (to 2000 local map points)
    nl = len(kl)
    z = rng.uniform(2, 10, nl)
    xyz = np.stack([(kl["x"] - INTR[2]) / INTR[0] * z, (kl["y"] - INTR[3]) / INTR[1] * z, z], 1)
    n_extra = 2000 - nl
    src = rng.integers(0, nl, n_extra)
    flips = np.packbits(rng.random((n_extra, 256)) < 0.08, axis=1, bitorder="little")
    mp_desc = np.concatenate([dl, dl[src] ^ flips])
    mp_xy = np.concatenate([np.stack([kl["x"], kl["y"]], 1), np.stack([kl["x"][src], kl["y"][src]], 1) + rng.normal(0, 6, (n_extra, 2))])
    mp_oct = np.concatenate([kl["octave"], kl["octave"][src]]).astype("i4")
    xyz = np.concatenate([xyz, xyz[src] + rng.normal(0, 0.05, (n_extra, 3))]).astype(np.float32).astype(np.float64)
    last_ids = np.where(rng.random(nl) < 0.9, np.arange(nl), -1).astype("i4")
    return dict(ex=ex, cur_img=cur_img, kl=kl, dl=dl, kc=kc, dc=dc, mp_desc=mp_desc, mp_xy=mp_xy, mp_oct=mp_oct, xyz=xyz, last_ids=last_ids,
                sf=ex.GetScaleFactors(), is2=ex.GetInverseScaleSigmaSquares())


def frame_args(W):
    kl = W["kl"]
    ids = W["last_ids"]
    u = (kl["x"] + SHIFT[1]).astype("f4"); v = (kl["y"] + SHIFT[0]).astype("f4")
    valid = (ids >= 0) & (u >= 0) & (u < 752) & (v >= 0) & (v < 480)
    return valid, u, v, W["mp_desc"][np.maximum(ids, 0)], np.ones(len(u), bool)


def local_args(W, ids):
    px = (W["mp_xy"][:, 0] + SHIFT[1]).astype("f4"); py = (W["mp_xy"][:, 1] + SHIFT[0]).astype("f4")
    nm = len(px)
    in_view = (px >= 0) & (px < 752) & (py >= 0) & (py < 480)
    in_view[ids[ids >= 0]] = False
    return in_view, W["mp_oct"], np.full(nm, 0.999, "f4"), px, py, W["mp_desc"], np.ones(nm, bool), ids >= 0


def pose_host(W, view, ids, pose, ctx):
    has = ids >= 0
    p, o, n = Optimizer.PoseOptimizationClient(pose[None], INTR[None], np.array([0, has.sum()], "i4"), W["xyz"][ids[has]],
                                               np.stack([view.kx[has], view.ky[has]], 1).astype("f8"), W["is2"][view.oct[has]].astype("f8"),
                                               ctx=ctx)
    full = np.zeros(len(ids), np.uint8); full[has] = o
    return p[0], full, int(n[0])


def chain_host(W, m_f, m_l, ctx):
    kps, desc, counts = W["ex"].extract_batch(W["cur_img"][None])
    n = int(counts[0]); k = kps[0, :n]
    view = FrameGridView(k["x"], k["y"], k["octave"], desc[0, :n])
    valid, u, v, md, ho = frame_args(W)
    nb, mb, _ = m_f.SearchByProjectionFrame(view, k["angle"], W["sf"], valid, u, v, W["kl"]["octave"], W["kl"]["angle"], md, ho,
                                            np.zeros(n, bool), 7.0)
    ids = np.where(mb >= 0, W["last_ids"][np.maximum(mb, 0)], -1).astype("i4")
    pose, outl, ni = pose_host(W, view, ids, np.array([0, 0, 0, 1, 0, 0, 0.0]), ctx)
    ids[outl != 0] = -1
    la = local_args(W, ids)
    na, ma, _ = m_l.SearchByProjection(view, W["sf"], *la, 1.0)
    ids[ma >= 0] = ma[ma >= 0]
    pose2, outl2, ni2 = pose_host(W, view, ids, pose, ctx)
    return nb, mb, pose, outl, na, ma, pose2, outl2, ni2


def chain_handle(W, m_f, m_l, last):
    W["ex"].extract_batch(W["cur_img"][None])
    with DeviceFrame.from_extract(W["ex"], 0) as cur:
        valid, u, v, md, ho = frame_args(W)
        nb, mb, _ = m_f.SearchByProjectionFrameHandle(cur, last, W["sf"], valid, u, v, md, ho, np.zeros(cur.n, bool), 7.0)
        pose, outl, ni = Optimizer.PoseOptimizationFrame(cur, np.array([0, 0, 0, 1, 0, 0, 0.0]), INTR, W["xyz"], W["is2"])
        ids = np.where(mb >= 0, W["last_ids"][np.maximum(mb, 0)], -1).astype("i4")
        ids[outl != 0] = -1
        cur.map_points = ids
        la = local_args(W, ids)
        na, ma, _ = m_l.SearchByProjectionHandle(cur, W["sf"], *la, 1.0)
        pose2, outl2, ni2 = Optimizer.PoseOptimizationFrame(cur, pose, INTR, W["xyz"], W["is2"])
    return nb, mb, pose, outl, na, ma, pose2, outl2, ni2


# cslam/conf/vi_euroc.yaml: the 752 x 480 camera with distortion
EUROC = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, k1=-0.28340811, k2=0.07395907, p1=0.00019359, p2=1.76187114e-05)
N_BATCH = 256


def setup_distorted(W, ctx, torch):
    """The inputs of (e) and (f): the current image and a batch of 256 in device memory, the last frame's handle with undistorted
    coordinates and a map made from them."""
    cam = Camera(**EUROC)
    b = cam.image_bounds(752, 480)
    ex = W["ex"]
    last_img = np.roll(W["cur_img"], (-SHIFT[0], -SHIFT[1]), axis=(0, 1))
    kl, dl = ex(last_img)
    last = DeviceFrame.from_extract(ex, 0, camera=cam, bounds=b, ctx=ctx)
    lx, ly = last.keypoints()
    rng = np.random.default_rng(2)
    nl = len(kl)
    z = rng.uniform(2, 10, nl)
    xyz = np.stack([(lx - INTR[2]) / INTR[0] * z, (ly - INTR[3]) / INTR[1] * z, z], 1).astype(np.float32).astype(np.float64)
    ids = np.where(rng.random(nl) < 0.9, np.arange(nl), -1).astype("i4")
    last.map_points = ids
    u = (lx + SHIFT[1]).astype("f4"); v = (ly + SHIFT[0]).astype("f4")
    valid = (ids >= 0) & (u >= b.min_x) & (u < b.max_x) & (v >= b.min_y) & (v < b.max_y)
    dev_cur = torch.from_numpy(W["cur_img"][None].copy()).cuda()
    batch = np.stack([np.roll(W["cur_img"], (k % 16, -(k // 16)), axis=(0, 1)) for k in range(N_BATCH)])
    dev_batch = torch.from_numpy(batch).cuda()
    torch.cuda.synchronize()
    return dict(cam=cam, b=b, last=last, ids=ids, xyz=xyz, args=(valid, u, v, dl, np.ones(nl, bool)), dev_cur=dev_cur, dev_batch=dev_batch)


def distorted_chain(W, D, m_f, ctx, new_route):
    ex, cam, b = W["ex"], D["cam"], D["b"]
    ex.extract_dev(D["dev_cur"].data_ptr(), 752, 480, 752, 752 * 480, 1)
    if new_route:
        cur = DeviceFrame.from_extract(ex, 0, camera=cam, bounds=b, ctx=ctx)
    else:
        kps = np.zeros((1, ex.max_per_image), _lib.KP_DTYPE); cnt = np.zeros(1, "i4")
        ctx.check(ctx.lib.ccm_orb_fetch(ctx.handle, _lib.ptr(kps), None, _lib.ptr(cnt)))      # count and keypoints, no descriptors
        n = int(cnt[0])
        kxu, kyu = cam.undistort(kps[0, :n]["x"], kps[0, :n]["y"])
        cur = DeviceFrame.from_extract(ex, 0, kxu, kyu, n=n, min_x=b.min_x, max_x=b.max_x, min_y=b.min_y, max_y=b.max_y, ctx=ctx)
    with cur:
        valid, u, v, md, ho = D["args"]
        nb, mb, _ = m_f.SearchByProjectionFrameHandle(cur, D["last"], W["sf"], valid, u, v, md, ho, np.zeros(cur.n, bool), 7.0)
        pose, outl, ni = Optimizer.PoseOptimizationFrame(cur, np.array([0, 0, 0, 1, 0, 0, 0.0]), INTR, D["xyz"], W["is2"])
    return nb, mb, pose, outl, ni


def build_handles(W, D, ctx, batched):
    """(f): the timed part makes the 256 handles and waits for the device; the check and the release are outside it."""
    ex, cam, b = W["ex"], D["cam"], D["b"]
    t0 = time.perf_counter()
    if batched:
        hs = DeviceFrame.batch_from_extract(ex, 0, N_BATCH, cam, b, ctx=ctx)
    else:
        hs = [DeviceFrame.from_extract(ex, k, camera=cam, bounds=b, ctx=ctx) for k in range(N_BATCH)]
    ctx.sync()
    dt = time.perf_counter() - t0
    res = tuple(x for k in (0, 17, N_BATCH - 1) for x in hs[k].keypoints() + hs[k].grid()) + (sum(h.n for h in hs),)
    for h in hs:
        h.close()
    return dt, res


def same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return bool(np.array_equal(np.asarray(a), np.asarray(b)))


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "n": len(t)}


def main():
    import torch                                                   # before the library is loaded: both then share one HIP runtime
    torch.cuda.init()
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--tag", default="r04")
    ap.add_argument("--out", default=None, help="output file (default profiles/<tag>_tracking_chain.json)")
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    W = setup(ctx)
    kc, dc, kl = W["kc"], W["dc"], W["kl"]
    view = FrameGridView(kc["x"], kc["y"], kc["octave"], dc)
    m_f = ORBmatcher(0.9, True, ctx=ctx); m_l = ORBmatcher(0.8, ctx=ctx)
    W["ex"](np.roll(W["cur_img"], (-SHIFT[0], -SHIFT[1]), axis=(0, 1)))          # the last image's extract -> its handle
    last = DeviceFrame.from_extract(W["ex"], 0, ctx=ctx)
    last.map_points = W["last_ids"]
    cur = DeviceFrame(view, kc["angle"], ctx=ctx)
    cur_pose = DeviceFrame(view, kc["angle"], ctx=ctx)                         # (c): its map points stay those of (b)
    n = len(kc)
    # (a) inputs: the frame already holds the motion-model matches of (b)
    valid, u, v, md, ho = frame_args(W)
    nb, mb, _ = m_f.SearchByProjectionFrame(view, kc["angle"], W["sf"], valid, u, v, kl["octave"], kl["angle"], md, ho, np.zeros(n, bool), 7.0)
    ids_b = np.where(mb >= 0, W["last_ids"][np.maximum(mb, 0)], -1).astype("i4")
    la = local_args(W, ids_b)
    pose0 = np.array([0, 0, 0, 1, 0, 0, 0.0])
    cases = {
        "a_search_by_projection_frame_mappoints": (
            lambda: m_l.SearchByProjection(view, W["sf"], *la, 1.0),
            lambda: m_l.SearchByProjectionHandle(cur, W["sf"], *la, 1.0)),
        "b_search_by_projection_current_last": (
            lambda: m_f.SearchByProjectionFrame(view, kc["angle"], W["sf"], valid, u, v, kl["octave"], kl["angle"], md, ho, np.zeros(n, bool), 7.0),
            lambda: m_f.SearchByProjectionFrameHandle(cur, last, W["sf"], valid, u, v, md, ho, np.zeros(n, bool), 7.0)),
        "c_pose_one_frame": (
            lambda: pose_host(W, view, ids_b, pose0, ctx),
            lambda: Optimizer.PoseOptimizationFrame(cur_pose, pose0, INTR, W["xyz"], W["is2"])),
        "d_chain": (
            lambda: chain_host(W, m_f, m_l, ctx),
            lambda: chain_handle(W, m_f, m_l, last)),
    }
    D = setup_distorted(W, ctx, torch)
    cases["e_distorted_extract_handle_match_pose"] = (
        lambda: distorted_chain(W, D, m_f, ctx, False),
        lambda: distorted_chain(W, D, m_f, ctx, True))
    cur.map_points = ids_b
    cur_pose.map_points = ids_b
    result = {"workload": {"image": [752, 480], "features": n, "local_map_points": len(W["xyz"]), "reps": a.reps, "warmup": a.warmup},
              "cases": {}}
    for name, (old, new) in cases.items():
        for _ in range(a.warmup):
            old(); new()
        t_old, t_new, mismatches = [], [], 0
        for r in range(a.reps):
            first_old = r % 2 == 0                                 # alternate which path goes first
            for which in ((0, 1) if first_old else (1, 0)):
                f = old if which == 0 else new
                t0 = time.perf_counter(); res = f(); t1 = time.perf_counter()
                (t_old if which == 0 else t_new).append(t1 - t0)
                if which == 0: ro = res
                else: rn = res
            mismatches += not same(tuple(ro), tuple(rn))
        ko, kn = ("todays_route", "new_route") if name.startswith("e_") else ("host_buffers", "handle")
        result["cases"][name] = {ko: stats(t_old), kn: stats(t_new), "mismatching_reps": mismatches}
        print("%-42s %s %.4f ms [%.4f, %.4f]   %s %.4f ms [%.4f, %.4f]   mismatches %d" % (
            name, ko, *(result["cases"][name][ko][k] for k in ("median_ms", "p10_ms", "p90_ms")),
            kn, *(result["cases"][name][kn][k] for k in ("median_ms", "p10_ms", "p90_ms")), mismatches), flush=True)
    result["cases"]["e_distorted_extract_handle_match_pose"]["matches"] = int(distorted_chain(W, D, m_f, ctx, True)[0])
    # (f) 256 handles of one extract: 256 calls against one batched call, alternating; the time is taken inside build_handles
    W["ex"].extract_dev(D["dev_batch"].data_ptr(), 752, 480, 752, 752 * 480, N_BATCH)
    ctx.sync()
    reps_f = max(20, a.reps // 10)
    for _ in range(3):
        build_handles(W, D, ctx, False); build_handles(W, D, ctx, True)
    t_old, t_new, mismatches = [], [], 0
    for r in range(reps_f):
        for which in ((0, 1) if r % 2 == 0 else (1, 0)):
            dt, res = build_handles(W, D, ctx, which == 1)
            (t_old if which == 0 else t_new).append(dt)
            if which == 0: ro = res
            else: rn = res
        mismatches += not same(ro, rn)
    name = "f_build_256_handles"
    result["cases"][name] = {"calls_256": stats(t_old), "one_batched_call": stats(t_new), "mismatching_reps": mismatches,
                             "features_total": int(ro[-1])}
    print("%-42s 256 calls %.4f ms [%.4f, %.4f]   batched %.4f ms [%.4f, %.4f]   mismatches %d" % (
        name, *(result["cases"][name]["calls_256"][k] for k in ("median_ms", "p10_ms", "p90_ms")),
        *(result["cases"][name]["one_batched_call"][k] for k in ("median_ms", "p10_ms", "p90_ms")), mismatches), flush=True)
    last.close(); cur.close(); cur_pose.close(); D["last"].close()
    out = a.out or os.path.join(ROOT, "profiles", "%s_tracking_chain.json" % a.tag)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: tuple(x["median_ms"] if isinstance(x, dict) else x for x in list(v.values())[:3]) for k, v in result["cases"].items()}))
    bad = sum(v["mismatching_reps"] for v in result["cases"].values())
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
