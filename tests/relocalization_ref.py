"""Relocalisation restated for the tests, from the reference's text and independent of the library.

`RelocDatabase` adds KeyFrameDatabase::DetectRelocalizationCandidates (cslam/src/Database.cpp:329-439) to the literal inverted-file
walk of kfdb_ref.RefDatabase, statement by statement, with the fields it keeps on the keyframes (`mnRelocWords`, `mRelocQuery`,
`mRelocScore`).  The reference leaves mRelocScore uninitialised (src/KeyFrame.cpp:56); here a keyframe starts with 0 when it is
made (the one stated deviation), and a keyframe that is erased and added again is a new keyframe.

`pnp_correspondences` is the constructor loop of PnPsolver (src/PnPSolver.cpp:69-91) over a frame's arrays and a table's rows: what
ccm_pnp_solver_create_frames gathers on the device, as the arrays ccm_pnp_solver_create takes.

`reloc_queries` / `reloc_search` restate the relocalisation overload of ORBmatcher::SearchByProjection (src/ORBmatcher.cpp:1478-1605)
in the arithmetic of search_local_points_ref.py, with the CPU oracle as the windowed matcher; `relocalize_candidate` replays one
candidate of ORB-SLAM's Relocalization from the PnP pose to the verdict with a pose callback (track_motion_model_ref.oracle_pose's
kind).  Nothing here touches the GPU."""
import numpy as np

import kfdb_ref as K
import search_local_points_ref as R

F = np.float32


class KF(K.KF):
    def __init__(self, key, ids, vals, map_id=0, client=0):
        super().__init__(key, ids, vals, map_id, client)
        self.mnRelocWords = 0; self.mRelocQuery = None; self.mRelocScore = F(0)


class RelocDatabase(K.RefDatabase):
    def detect_reloc(self, frame_id, ids, vals):
        """DetectRelocalizationCandidates(Frame&): frame_id = F.mId, (ids, vals) = F.mBowVec in key order."""
        out = {"listed": [], "min_common_words": 0, "shortlist": [], "candidates": []}
        sharing = []
        for w in ids:                                                            # :337-352
            for k in self.inverted.get(int(w), []):
                if k.mRelocQuery != frame_id:
                    k.mnRelocWords = 0
                    k.mRelocQuery = frame_id
                    sharing.append(k)
                k.mnRelocWords += 1
        out["listed"] = [k.key for k in sharing]
        if not sharing:                                                          # :354
            return out
        max_common = 0
        for k in sharing:                                                        # :358-363
            if k.mnRelocWords > max_common:
                max_common = k.mnRelocWords
        min_common = int(F(max_common) * F(0.8))                                 # :365
        score_and_match = []
        for k in sharing:                                                        # :372-383
            if k.mnRelocWords > min_common:
                si = F(K.l1_score(ids, vals, k.ids, k.vals))
                k.mRelocScore = si
                score_and_match.append((si, k))
        if not score_and_match:                                                  # :385
            return out
        out["min_common_words"] = min_common
        out["shortlist"] = [k.key for _, k in score_and_match]
        acc_and_match = []
        best_acc = F(0)                                                          # :389
        for si, k in score_and_match:                                            # :392-417
            best, acc, best_kf = si, si, k
            for k2 in k.best_covis[:10]:
                if k2.mRelocQuery != frame_id:                                   # :403
                    continue
                acc = F(acc + k2.mRelocScore)
                if k2.mRelocScore > best:
                    best_kf, best = k2, k2.mRelocScore
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        retain = F(F(0.75) * best_acc)                                           # :420
        out["acc"] = [a for a, _ in acc_and_match]; out["retain"] = retain
        added = set()
        for acc, k in acc_and_match:                                             # :424-436
            if acc > retain and k.key not in added:
                out["candidates"].append(k.key)
                added.add(k.key)
        return out


def pnp_correspondences(kx, ky, octave, level_sigma2, mp_id, pos, usable):
    """PnPsolver's constructor (:69-91) for one candidate: vpMapPointMatches[i] = table slot mp_id[i] (-1: none), usable[slot] =
    "not bad".  Returns (P2D [N][2], P3Dw [N][3], sigma2 [N], kp_index [N]) as float32 / int32, in feature order."""
    idx = np.array([i for i in range(len(mp_id)) if mp_id[i] >= 0 and usable[mp_id[i]]], "i4")
    s = np.asarray(mp_id, "i4")[idx]
    P2D = np.stack([np.asarray(kx, "f4")[idx], np.asarray(ky, "f4")[idx]], 1).astype("f4").reshape(-1, 2)
    return P2D, np.asarray(pos, "f4").reshape(-1, 3)[s], np.asarray(level_sigma2, "f4")[np.asarray(octave)[idx]], idx


# ------------------------------------------------------------------------------------- the relocalisation SearchByProjection
REASONS = ("query", "no id", "bad", "found", "not finite", "u outside", "v outside", "distance")
QUERY, NO_ID, BAD_SLOT, FOUND, NOT_FINITE, U_OUT, V_OUT, DISTANCE = range(8)


def reloc_queries(kf_ids, rows, Tcw, Ow, found=(), intr=R.INTR, bounds=R.BOUNDS, log_sf=R.LOG_SF, n_levels=R.N_LEVELS):
    """The first half of the loop of SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cpp:1494-1529)
    for every keyframe feature: dict(reason [N_kf] -- the first test that rejects, in the reference's order --, valid, u, v, level,
    desc, dist).  No depth test: a point behind the camera is projected like any other.  u, v and level are 0 where the feature is no
    query.  The arithmetic is R.frustum's (Pc and the norm summed in double and stored as float, the rest float left to right)."""
    ids = np.asarray(kf_ids, "i4")
    flags = np.asarray(rows["flags"], np.uint8)
    has = ids >= 0
    assert (flags[ids[has]] & R.LIVE).all()
    safe = np.maximum(ids, 0)
    fr = R.frustum(np.asarray(rows["pos"], "f4")[safe], np.asarray(rows["normal"], "f4")[safe], np.asarray(rows["min_dist"], "f4")[safe],
                   np.asarray(rows["max_dist"], "f4")[safe], Tcw, Ow, intr, bounds, 0.5, log_sf, n_levels)
    u, v, dist = fr["u"], fr["v"], fr["dist"]
    x0, x1, y0, y1 = [F(b) for b in bounds]
    mn = np.asarray(rows["min_dist"], "f4")[safe]; mx = np.asarray(rows["max_dist"], "f4")[safe]
    in_found = np.isin(ids, np.asarray(list(found), "i4"))
    reason = np.zeros(len(ids), "i4")
    with np.errstate(all="ignore"):
        for k, rej in ((DISTANCE, (dist < F(0.8) * mn) | (dist > F(1.2) * mx)), (V_OUT, (v < y0) | (v > y1)), (U_OUT, (u < x0) | (u > x1)),
                       (NOT_FINITE, ~(np.isfinite(u) & np.isfinite(v))), (FOUND, in_found), (BAD_SLOT, (flags[safe] & R.BAD) != 0), (NO_ID, ~has)):
            reason[rej] = k                       # the earliest test wins: assigned last
    ok = reason == QUERY
    return dict(reason=reason, valid=ok, u=np.where(ok, u, F(0)).astype("f4"), v=np.where(ok, v, F(0)).astype("f4"),
                level=np.where(ok, fr["level"], 0).astype("i4"), desc=np.asarray(rows["desc"], np.uint8)[safe], dist=dist)


def reloc_search(oracle, cur, cur_angle, cur_ids, kf_angle, kf_ids, rows, Tcw, Ow, scale, th, orb_dist, check_ori=True, found=None, **kw):
    """The whole overload, sequentially: the queries above, then the window search, the acceptance in keyframe-feature order and the
    rotation histogram through the CPU oracle's SearchByProjection(Frame, Frame) fed with level as the query's octave (radius = th *
    scale[level], levels level-1 .. level+1, :1532-1534), every query flagged 1 and a current feature occupied when it holds any id
    (:1547).  found = None: every id the current frame holds.  Returns the queries dict plus n_matches, match [N_cur], mp_id [N_cur]."""
    cur_ids = np.asarray(cur_ids, "i4")
    if found is None:
        found = cur_ids[cur_ids >= 0]
    q = reloc_queries(kf_ids, rows, Tcw, Ow, found, **kw)
    n = len(cur.kx)
    if n == 0 or len(q["valid"]) == 0:
        return dict(q, n_matches=0, match=np.full(n, -1, "i4"), mp_id=cur_ids.copy())
    nm, match, _ = oracle.search_by_projection_frame(cur.kx, cur.ky, cur.oct, cur.desc, cur_angle, cur.min_x, cur.min_y, cur.inv_w, cur.inv_h,
                                                     scale, q["valid"], q["u"], q["v"], q["level"], kf_angle, q["desc"],
                                                     np.ones(len(q["valid"]), np.uint8), (cur_ids >= 0).astype(np.uint8), F(th), check_ori,
                                                     orb_dist=orb_dist)
    ids = np.where(match >= 0, np.asarray(kf_ids, "i4")[np.maximum(match, 0)], cur_ids).astype("i4")
    return dict(q, n_matches=int(nm), match=match, mp_id=ids)


# ------------------------------------------------------------------------------------- one candidate, from the PnP pose to the verdict
POSE1, SEARCH1, POSE2, SEARCH2, POSE3 = 1, 2, 4, 8, 16


def pose_to_camera(pose7):
    """Tcw [3][4] float32 and Ow [3] float32 of an SE3Quat (qx, qy, qz, qw, t): Converter::toCvMat -- the quaternion's rotation matrix
    in double, each entry and the translation narrowed to float -- and Ow = -Rcw^T tcw on the float matrices, the three products summed
    left to right in double and narrowed once (KeyFrame::SetPose, src/KeyFrame.cpp:299-302)."""
    x, y, z, w = [float(v) for v in pose7[:4]]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    Rm = np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])
    T = np.concatenate([Rm, np.asarray(pose7[4:7], "f8")[:, None]], 1).astype("f4")
    Td = T.astype("f8")
    Ow = np.array([((-Td[0, r]) * Td[0, 3] - Td[1, r] * Td[1, 3]) - Td[2, r] * Td[2, 3] for r in range(3)]).astype("f4")
    return T, Ow


def relocalize_candidate(oracle, pose, cur, cur_angle, kf_angle, kf_ids, rows, feature, slot, scale, min_good=10, enough=50, narrow_above=30,
                         th1=10.0, dist1=100, th2=3.0, dist2=64, check_ori=True, **kw):
    """The candidate loop's body of ORB-SLAM's Tracking::Relocalization behind PnPsolver::iterate, sequentially, in its nesting.  pose:
    a callback (ids [N_cur], pose7 or None = the start pose) -> (pose7, outlier [N_cur], n_inliers); (feature, slot): the PnP inliers.
    Returns dict(success, n_good, stages, n_add1, n_add2, pose7, mp_id, outlier)."""
    n = len(cur.kx)
    ids = np.full(n, -1, "i4")
    ids[np.asarray(feature, "i4")] = np.asarray(slot, "i4")                      # 1.
    found = list(np.asarray(slot, "i4"))
    out = dict(success=False, stages=POSE1, n_add1=0, n_add2=0)
    p7, outl, good = pose(ids, None)                                             # 2.
    if good >= min_good:
        ids = np.where(np.asarray(outl) != 0, -1, ids).astype("i4")

        def search(th, dist, fnd):
            T, Ow = pose_to_camera(p7)
            s = reloc_search(oracle, cur, cur_angle, ids, kf_angle, kf_ids, rows, T, Ow, scale, th, dist, check_ori, fnd, **kw)
            return s["n_matches"], s["mp_id"]
        if good < enough:
            out["n_add1"], ids = search(th1, dist1, found); out["stages"] |= SEARCH1           # 3.
            if good + out["n_add1"] >= enough:
                p7, outl, good = pose(ids, p7); out["stages"] |= POSE2                          # 4.
                if narrow_above < good < enough:
                    out["n_add2"], ids = search(th2, dist2, None); out["stages"] |= SEARCH2     # 5.
                    if good + out["n_add2"] >= enough:
                        p7, outl, good = pose(ids, p7); out["stages"] |= POSE3                  # 6.
                        ids = np.where(np.asarray(outl) != 0, -1, ids).astype("i4")
        out["success"] = good >= enough                                                         # 7.
    out.update(n_good=int(good), pose7=p7, mp_id=ids, outlier=np.asarray(outl, np.uint8))
    return out
