"""Relocalisation on frame handles and the map-point table against the array route it replaces, stage by stage.

Workload: a lost frame of 1000 features and five candidate keyframes of 1000 features that all see it (tests/frame_bow_ref.py: the
keyframe's own camera is the world frame), every candidate's map points in one table.  Per repetition, in one process after a
warm-up, the two routes alternate and their results are compared:
  candidates   the host replay of DetectRelocalizationCandidates over the arrays of one query: the two library calls
               ccm_kfdb_shortlist + ccm_kfdb_reloc_candidates, the neighbour array laid out beforehand.  The parent has no entry point
               for it, so there is no old figure.
  create       old: ccm_pnp_solver_create from P2D / P3Dw / sigma2 / kp_index collected on the host (24 bytes per correspondence);
               new: ccm_pnp_solver_create_frames (8 bytes).  Collecting the arrays is outside the clock on both routes.
  refinement   one candidate from the PnP pose to the verdict with 40 inliers and `enough` set to what the first search just reaches;
               the stages that run are recorded in the JSON (workload.stages, CCM_RELOC_* bits).
               old: ccm_frame_set_map_points, ccm_frame_pose_optimize, and per search the projection of every keyframe point on the
               host (numpy, tests/relocalization_ref.py: charged to the old route, it is what that route asks of its caller) uploaded
               into ccm_search_by_projection_frame; new: one ccm_frame_relocalize_candidate.
Timed with the host clock around calls that end in a stream synchronisation.  Only the times are measured: the uploaded bytes are
computed from the staging layouts and the synchronisation counts follow from the stages that ran.  The old refinement's time includes
the Python that drives it.  Output: profiles/relocalization.json and one line.

    python tools/bench_relocalization.py [--reps 30] [--warmup 5]
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

import frame_bow_ref as fb  # noqa: E402
import relocalization_ref as RR  # noqa: E402
import search_local_points_ref as R  # noqa: E402
from motioncheck_ccm_slam_amd import _lib, database as D  # noqa: E402
from motioncheck_ccm_slam_amd.frame import DeviceFrame  # noqa: E402
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher  # noqa: E402
from motioncheck_ccm_slam_amd.optimizer import Optimizer  # noqa: E402
from motioncheck_ccm_slam_amd.pnpsolver import PnPSolver, make_draws  # noqa: E402
from motioncheck_ccm_slam_amd.tracking import MapPointTable, Tracking  # noqa: E402
from motioncheck_ccm_slam_amd.vocabulary import ORBVocabulary  # noqa: E402

COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")
INTR = np.array(R.INTR, "f8")
N, K_CAND, N_INLIERS = 1000, 5, 40


def seg(n):
    return (n + 63) & ~63


def stats(ts):
    a = np.sort(np.asarray(ts)) * 1e3
    return dict(median_ms=float(np.median(a)), p10_ms=float(a[int(0.1 * (len(a) - 1))]), p90_ms=float(a[int(0.9 * (len(a) - 1))]), min_ms=float(a[0]),
                max_ms=float(a[-1]), n=len(a))


class ArrayRoute:
    def __init__(self, ctx, cur):
        self.ctx, self.cur, self.calls = ctx, cur, 0

    def search_by_projection_frame(self, kx, ky, octv, desc, angle, min_x, min_y, inv_w, inv_h, scale, valid, u, v, lo, la, md, ho, occ, th, check_ori,
                                   orb_dist=100):
        self.calls += 1
        return ORBmatcher(0.9, check_ori, ctx=self.ctx).SearchByProjectionFrame(self.cur, angle, scale, valid, u, v, lo, la, md, ho, occ, float(th), orb_dist)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30); ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    tr = fb.tree()
    voc = ORBVocabulary(fb.K, fb.L, *tr, ctx=ctx)
    kf = fb.make_kf(tr, 3, N); cur = fb.make_view(tr, kf, 1, N)
    cap = K_CAND * N
    rows = R.random_points(cap, 5); rows["flags"][:] = R.LIVE | R.HAS_OBS
    d = np.linalg.norm(kf["xyz"], axis=1); mx = d * 1.2 ** (kf["oct"].astype("f8") - 0.5)
    for k in range(K_CAND):
        s = slice(k * N, (k + 1) * N)
        rows["pos"][s] = kf["xyz"].astype("f4"); rows["desc"][s] = kf["desc"]; rows["max_dist"][s] = mx.astype("f4"); rows["min_dist"][s] = (mx / 1.2 ** 7).astype("f4")
    ids = [np.where(kf["ids"] >= 0, kf["ids"] + k * N, -1).astype("i4") for k in range(K_CAND)]
    sig2 = (R.SCALE * R.SCALE).astype("f4"); inv_sig2 = (np.float32(1) / sig2).astype("f4")
    cv = FrameGridView(cur["kx"], cur["ky"], cur["oct"], cur["desc"])
    kv = FrameGridView(kf["kx"], kf["ky"], kf["oct"], kf["desc"])
    t = MapPointTable(cap, ctx=ctx); t.update(np.arange(cap), **{c: rows[c] for c in COLS})
    hc = DeviceFrame(cv, cur["angle"], ctx=ctx); hs = DeviceFrame(cv, cur["angle"], ctx=ctx)
    hk = [DeviceFrame(kv, kf["angle"], ctx=ctx) for _ in range(K_CAND)]
    for h, i in zip(hk, ids):
        h.map_points = i; h.compute_bow(voc, 3, outputs=False)
    hc.compute_bow(voc, 3, outputs=False)
    nm, m12 = ORBmatcher(0.75, True, ctx=ctx).SearchByBoWFrames(hc, hk, valid1=np.ones(hc.n, np.uint8))
    vp = [np.where(m12[k] >= 0, ids[k][np.maximum(m12[k], 0)], -1).astype("i4") for k in range(K_CAND)]
    per = [RR.pnp_correspondences(cur["kx"], cur["ky"], cur["oct"], sig2, v, rows["pos"], np.ones(cap, bool)) for v in vp]
    first = np.concatenate([[0], np.cumsum([len(p[3]) for p in per])]).astype("i4")
    cat = lambda j: np.concatenate([p[j] for p in per])  # noqa: E731
    P2D, P3D, S2, feat = cat(0), cat(1), cat(2), cat(3).astype("i4")
    slot = np.concatenate([v[p[3]] for v, p in zip(vp, per)]).astype("i4")
    Kf = np.tile(INTR.astype("f4"), (K_CAND, 1))
    draws = make_draws(np.random.default_rng(9), np.diff(first), 340)
    T = int(first[-1])

    # the database stage: twelve-word vectors would say nothing; 2000 stored entries of the size the query kernel delivers
    rng = np.random.default_rng(1)
    n_slots = 2000
    words = rng.integers(0, 60, n_slots).astype("i4"); score = rng.uniform(0, 0.2, n_slots); fw = rng.integers(0, 500, n_slots).astype("i4")
    seq = np.arange(n_slots, dtype="i8"); reloc = np.zeros(n_slots, "f4")
    nbr = rng.integers(0, n_slots, (n_slots, D.NEIGHBOURS))

    # Only the two library calls are inside the clock: the shortlist is the same on every repetition, so the neighbour rows of its
    # entries (the caller's covisibility look-ups) are laid out once, outside.
    lib = _lib.load()
    short0, _ = D.shortlist(words, score, fw, seq, np.ones(n_slots, np.uint8), -np.inf, -1)
    nb0 = np.ascontiguousarray(nbr[short0], "i4"); all_on = np.ones(n_slots, np.uint8)
    sl_buf = np.zeros(n_slots, "i4"); cand_buf = np.zeros(n_slots, "i4"); mcw = np.zeros(1, "i4")
    p = _lib.ptr

    def candidates():
        ns = lib.ccm_kfdb_shortlist(n_slots, p(words), p(score), p(fw), p(seq), p(all_on), -1, -np.inf, n_slots, p(sl_buf), p(mcw))
        assert ns == len(short0)
        return lib.ccm_kfdb_reloc_candidates(n_slots, p(words), p(score), p(seq), ns, p(sl_buf), p(nb0), p(reloc), p(cand_buf))

    def create(frames):
        s = (PnPSolver.from_frames(hc, t, first, Kf, feat, slot, sig2, draws, reserve=40, ctx=ctx) if frames else
             PnPSolver(first, np.full(K_CAND, hc.n, "i4"), Kf, P2D, P3D, S2, feat, draws, reserve=40, ctx=ctx))
        s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
        s._ensure()
        return s

    Tpnp = np.eye(4, dtype="f4"); Tpnp[:3, 3] = [0.05 + 0.02, 0.02 - 0.01, 0.03]
    start = np.zeros(7); assert _lib.load().ccm_pose_from_mat4f(_lib.ptr(Tpnp), _lib.ptr(start)) == 0
    f_in = per[0][3][:N_INLIERS].astype("i4"); s_in = vp[0][f_in]
    xyz = rows["pos"].astype("f8")
    kw = dict(dist1=35, narrow_above=0)
    probe = Tracking.RelocalizeCandidate(hc, hk[0], t, Tpnp, f_in, s_in, INTR, R.SCALE, inv_sig2, enough=10 ** 6, **kw)
    kw["enough"] = probe.n_good + probe.n_add1           # search 1 just reaches it, so the second pose runs
    route = ArrayRoute(ctx, cv)

    def pose_cb(ids_, p7):
        hs.map_points = ids_
        return Optimizer.PoseOptimizationFrame(hs, start if p7 is None else p7, INTR, xyz, inv_sig2, ctx=ctx)

    def refine(new):
        if new:
            return Tracking.RelocalizeCandidate(hc, hk[0], t, Tpnp, f_in, s_in, INTR, R.SCALE, inv_sig2, **kw)
        return RR.relocalize_candidate(route, pose_cb, cv, cur["angle"], kf["angle"], ids[0], rows, f_in, s_in, R.SCALE, **kw)

    times = {k: [] for k in ("candidates_new", "create_old", "create_new", "refine_old", "refine_new")}
    stages = 0
    for rep in range(a.warmup + a.reps):
        rec = rep >= a.warmup
        t0 = time.perf_counter(); candidates(); t1 = time.perf_counter()
        so = create(False); t2 = time.perf_counter(); sn = create(True); t3 = time.perf_counter()
        for k in range(K_CAND):
            ho, hn = so.hypotheses(k), sn.hypotheses(k)
            assert all(np.ascontiguousarray(ho[key]).tobytes() == np.ascontiguousarray(hn[key]).tobytes() for key in ho), ("create", rep, k)
        so.close(); sn.close()
        t4 = time.perf_counter(); ro = refine(False); t5 = time.perf_counter(); rn = refine(True); t6 = time.perf_counter()
        assert (ro["mp_id"] == rn.mp_id).all() and ro["n_good"] == rn.n_good and ro["stages"] == rn.stages and np.asarray(ro["pose7"]).tobytes() == rn.pose7.tobytes(), ("refine", rep)
        stages = rn.stages
        if rec:
            for key, v in zip(times, (t1 - t0, t2 - t1, t3 - t2, t5 - t4, t6 - t5)):
                times[key].append(v)
    n_search = bin(stages & 10).count("1"); n_pose = bin(stages & 21).count("1")
    window = seg(4 * N) + seg(N) + 5 * seg(4 * N) + seg(32 * N) + 2 * seg(N) + 2 * seg(4 * N)      # frame grid side is resident only on handles: the array overload uploads the queries
    out = dict(workload=dict(n_cur=N, n_kf=N, candidates=K_CAND, correspondences=T, inliers=N_INLIERS, stages=stages, kfdb_slots=n_slots),
               candidates=dict(new=stats(times["candidates_new"]), old=None),
               create=dict(old=stats(times["create_old"]), new=stats(times["create_new"]), upload_bytes_computed=dict(old=24 * T, new=8 * T + 64),
                           synchronisations_by_construction=dict(old=2, new=2)),
               refinement=dict(old=stats(times["refine_old"]), new=stats(times["refine_new"]),
                               upload_bytes_computed=dict(old=n_search * window + n_pose * (seg(56) + seg(32) + seg(32) + 24 * cap) + n_pose * 4 * N,
                                                 new=seg(56) + seg(32) + 64 + 2 * seg(4 * N_INLIERS)),
                               synchronisations_by_construction=dict(old_at_least=n_search + n_pose, new=n_search + n_pose)),
               note="only the *_ms figures are measured.  The old refinement drives the array entry points from Python (tests/relocalization_ref.py): its "
                    "time includes the numpy projection and the Python control flow, so it is an upper bound for that route, not a library figure.  Upload bytes "
                    "are computed from the staging layouts (the per-hypothesis and per-solver records of create are the same on both routes and left "
                    "out); the synchronisation counts follow from the stages that ran, they are not counted at run time.")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "relocalization.json"), "w"), indent=1)
    print(json.dumps({k: (v["new"]["median_ms"], None if not v.get("old") else v["old"]["median_ms"]) for k, v in out.items() if k in ("candidates", "create", "refinement")}))


if __name__ == "__main__":
    main()
