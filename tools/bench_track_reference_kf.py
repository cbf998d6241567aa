"""Tracking::TrackReferenceKeyFrame and the SearchByBoW loop of loop / map matching: host arrays vs frame handles.

Workload: a synthetic 4-level, 10-way vocabulary (tests/frame_bow_ref.py's shape), a reference keyframe of 1000 features and frames of
1000 features that see 80 % of it again.  Cases, each timed with the host clock around synchronised calls, the two paths alternating
inside one process after a warm-up:
  (a) the chain of src/Tracking.cpp:514-556 for one frame whose descriptors already lie in device memory:
        arrays:  ccm_voc_transform_dev + ccm_bow_vector + ccm_match_bow + ccm_pose_optimize (+ the host gathers between them)
        handles: ccm_frame_compute_bow + ccm_frame_search_by_bow + ccm_frame_pose_optimize (+ ccm_frame_set_map_points for the outliers)
  (b) SearchByBoW(KeyFrame, KeyFrame) of one keyframe against 20 candidates (src/LoopFinder.cpp:265):
        arrays:  20 ccm_match_bow calls;  handles: one ccm_search_by_bow_frames call
Every repetition's results are compared between the paths.  Output: profiles/<tag>_track_reference_kf.json and one summary line.

    python tools/bench_track_reference_kf.py [--reps 200] [--warmup 20] [--tag mi355x]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from motioncheck_ccm_slam_amd import _lib  # noqa: E402
from motioncheck_ccm_slam_amd.frame import DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher  # noqa: E402
from motioncheck_ccm_slam_amd.optimizer import Optimizer  # noqa: E402
from motioncheck_ccm_slam_amd.tracking import Tracking  # noqa: E402
from motioncheck_ccm_slam_amd.vocabulary import ORBVocabulary, synthetic_tree  # noqa: E402

K, L, LEVELSUP = 10, 4, 2
INTR = np.array([458.0, 457.0, 367.0, 248.0])
POSE0 = np.array([0, 0, 0, 1, 0, 0, 0.0])
INV_SIGMA2 = (1.0 / (1.2 ** np.arange(8)) ** 2).astype("f4")


def features(tree, rng, n):
    par, desc, w = tree
    flips = np.packbits(rng.random((n, 256)) < 0.1, axis=1, bitorder="little")
    return np.ascontiguousarray(desc[rng.integers(1, len(par), n)] ^ flips, np.uint8)


def make_kf(tree, rng, n):
    kx = rng.uniform(0, 752, n).astype("f4"); ky = rng.uniform(0, 480, n).astype("f4"); z = rng.uniform(2, 10, n)
    xyz = np.stack([(kx - INTR[2]) / INTR[0] * z, (ky - INTR[3]) / INTR[1] * z, z], 1).astype("f4").astype("f8")
    return dict(desc=features(tree, rng, n), angle=rng.uniform(0, 360, n).astype("f4"), kx=kx, ky=ky, oct=rng.integers(0, 8, n).astype("i4"),
                ids=np.where(rng.random(n) < 0.8, np.arange(n), -1).astype("i4"), xyz=xyz)


def make_view(tree, rng, kf, n, share=0.8):
    n1 = len(kf["desc"])
    src = np.full(n, -1, "i8"); m = min(int(share * n1), n)
    src[:m] = rng.permutation(n1)[:m]
    src = src[rng.permutation(n)]
    has = src >= 0
    d = features(tree, rng, n)
    d[has] = kf["desc"][src[has]] ^ np.packbits(rng.random((int(has.sum()), 256)) < 0.03, axis=1, bitorder="little")
    a = rng.uniform(0, 360, n).astype("f4")
    a[has] = np.mod(kf["angle"][src[has]] - np.float32(20.0), np.float32(360.0))
    kx = rng.uniform(0, 752, n).astype("f4"); ky = rng.uniform(0, 480, n).astype("f4"); octv = rng.integers(0, 8, n).astype("i4")
    P = kf["xyz"][src[has]] + np.array([0.05, 0.02, 0.0])
    kx[has] = (INTR[0] * P[:, 0] / P[:, 2] + INTR[2] + rng.normal(0, 0.5, len(P))).astype("f4")
    ky[has] = (INTR[1] * P[:, 1] / P[:, 2] + INTR[3] + rng.normal(0, 0.5, len(P))).astype("f4")
    octv[has] = kf["oct"][src[has]]
    return dict(desc=np.ascontiguousarray(d), angle=a, kx=kx, ky=ky, oct=octv, ids=np.where(rng.random(n) < 0.8, np.arange(n), -1).astype("i4"))


def handle(ctx, d, ids=None):
    f = DeviceFrame(FrameGridView(d["kx"], d["ky"], d["oct"], d["desc"]), d["angle"], ctx=ctx)
    if ids is not None:
        f.map_points = ids
    return f


def chain_arrays(ctx, voc, m, kf, f, desc_dev):
    """The only path the array entry points give: the frame's descriptors are on the device (as after ccm_orb_extract_dev), everything
    between the calls goes through the host."""
    n = len(f["desc"])
    wid, w, nid = voc.transform_features_dev(desc_dev, n, LEVELSUP)
    oid = np.zeros(n, "i4"); oval = np.zeros(n, "f8"); fv = np.full(n, -1, "i4")
    voc.lib.ccm_bow_vector(n, _lib.ptr(wid), _lib.ptr(w), _lib.ptr(nid), voc.weighting, voc.scoring, _lib.ptr(oid), _lib.ptr(oval), _lib.ptr(fv))
    nm, m12 = m.SearchByBoW(kf["desc"], kf["node"], kf["ids"] >= 0, kf["angle"], f["desc"], fv, f["angle"])
    match = np.full(n, -1, "i4")
    i1 = np.flatnonzero(m12 >= 0)
    match[m12[i1]] = i1
    ids = np.where(match >= 0, kf["ids"][np.maximum(match, 0)], -1).astype("i4")
    has = ids >= 0
    pose, o, ninl = Optimizer.PoseOptimizationClient(POSE0[None], INTR[None], np.array([0, has.sum()], "i4"), kf["xyz"][ids[has]],
                                                     np.stack([f["kx"][has], f["ky"][has]], 1).astype("f8"),
                                                     INV_SIGMA2[f["oct"][has]].astype("f8"), ctx=ctx)
    outl = np.zeros(n, np.uint8); outl[has] = o
    ids[outl != 0] = -1
    return nm, match, pose[0], outl, int(ninl[0]), ids


def chain_handles(voc, kfh, fh, kf):
    r = Tracking.TrackReferenceKeyFrame(fh, kfh, voc, POSE0, INTR, kf["xyz"], INV_SIGMA2, levelsup=LEVELSUP)
    return r["nmatches"], r["match"], r["pose"], r["outlier"], r["n_inliers"], r["mp_id"]


def same(a, b):
    return len(a) == len(b) and all(bool(np.array_equal(np.asarray(x), np.asarray(y))) for x, y in zip(a, b))


def stats(ts):
    t = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(t)), 4), "p10_ms": round(float(np.percentile(t, 10)), 4),
            "p90_ms": round(float(np.percentile(t, 90)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4), "n": len(t)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--candidates", type=int, default=20)
    ap.add_argument("--tag", default="mi355x")
    ap.add_argument("--out", default=None, help="output file (default profiles/<tag>_track_reference_kf.json)")
    a = ap.parse_args()
    import torch
    torch.cuda.init()                                                          # before the library: both then share one HIP runtime
    ctx = _lib.default_context(0)
    tree = synthetic_tree(K, L, seed=5, ragged=True)
    voc = ORBVocabulary(K, L, *tree, ctx=ctx)
    rng = np.random.default_rng(1)
    kf = make_kf(tree, rng, a.features)
    f = make_view(tree, rng, kf, a.features)
    cands = [make_view(tree, rng, kf, a.features, share=0.5) for _ in range(a.candidates)]
    kf["node"] = voc.transform(kf["desc"], LEVELSUP)[2]
    for c in cands:
        c["node"] = voc.transform(c["desc"], LEVELSUP)[2]
    desc_dev = torch.from_numpy(f["desc"]).cuda()                              # the frame's descriptor rows, device resident
    ctx.sync(); torch.cuda.synchronize()
    kfh = handle(ctx, kf, kf["ids"]); kfh.compute_bow(voc, LEVELSUP, outputs=False)
    fh = handle(ctx, f)
    chs = [handle(ctx, c, c["ids"]) for c in cands]
    for h in chs:
        h.compute_bow(voc, LEVELSUP, outputs=False)
    m_t = ORBmatcher(0.7, True, ctx=ctx); m_l = ORBmatcher(0.75, True, ctx=ctx)
    v1 = (kf["ids"] >= 0).astype(np.uint8); v2 = [(c["ids"] >= 0).astype(np.uint8) for c in cands]

    def loop_arrays():
        out = [m_l.SearchByBoW(kf["desc"], kf["node"], v1, kf["angle"], c["desc"], c["node"], c["angle"], valid2=v) for c, v in zip(cands, v2)]
        return np.array([o[0] for o in out], "i4"), np.stack([o[1] for o in out])

    cases = {
        "a_track_reference_keyframe": (lambda: chain_arrays(ctx, voc, m_t, kf, f, desc_dev.data_ptr()), lambda: chain_handles(voc, kfh, fh, kf)),
        "b_search_by_bow_1x%d_candidates" % a.candidates: (loop_arrays, lambda: m_l.SearchByBoWFrames(kfh, chs)),
    }
    result = {"workload": {"features": a.features, "candidates": a.candidates, "vocabulary_nodes": int(len(tree[0])), "levelsup": LEVELSUP,
                           "reps": a.reps, "warmup": a.warmup}, "cases": {}}
    for name, (old, new) in cases.items():
        for _ in range(a.warmup):
            old(); new()
        t_old, t_new, mismatches = [], [], 0
        for r in range(a.reps):
            for which in ((0, 1) if r % 2 == 0 else (1, 0)):                   # alternate which path goes first
                fn = old if which == 0 else new
                t0 = time.perf_counter(); res = fn(); t1 = time.perf_counter()
                (t_old if which == 0 else t_new).append(t1 - t0)
                if which == 0: ro = res
                else: rn = res
            mismatches += not same(tuple(ro), tuple(rn))
        result["cases"][name] = {"host_arrays": stats(t_old), "handles": stats(t_new), "mismatching_reps": mismatches,
                                 "matches": int(np.sum(ro[0]))}
        print("%-36s arrays %.4f ms [%.4f, %.4f]   handles %.4f ms [%.4f, %.4f]   mismatches %d" % (
            name, *(result["cases"][name]["host_arrays"][k] for k in ("median_ms", "p10_ms", "p90_ms")),
            *(result["cases"][name]["handles"][k] for k in ("median_ms", "p10_ms", "p90_ms")), mismatches), flush=True)
    for h in [kfh, fh] + chs:
        h.close()
    out = a.out or os.path.join(ROOT, "profiles", "%s_track_reference_kf.json" % a.tag)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fo:
        json.dump(result, fo, indent=1)
    print(json.dumps({k: (v["host_arrays"]["median_ms"], v["handles"]["median_ms"], v["mismatching_reps"]) for k, v in result["cases"].items()}))
    return 1 if sum(v["mismatching_reps"] for v in result["cases"].values()) else 0


if __name__ == "__main__":
    sys.exit(main())
