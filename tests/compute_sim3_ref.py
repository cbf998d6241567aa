"""numpy restatement of what ccm_sim3_solver_create_frames, ccm_optimize_sim3_table_frames and ccm_compute_sim3_table_frames
(include/ccm_hot.h "ComputeSim3 on handles") gather and list on the device, written from the reference's text: the constructor's loop
of Sim3Solver (src/Sim3Solver.cpp:30-83), the vertices and edges of OptimizeSim3 (src/Optimizer.cpp:920-999) and the round-robin of
LoopFinder::ComputeSim3 (src/LoopFinder.cpp:284-346); and the scenes the tests use.  On top of sim3_table_ref.py (the table, the
"matrix product", SearchBySim3's projections), window_matcher_ref.py (its selections) and sim3_solver_ref.py (iterate's bookkeeping).
Shared by test_compute_sim3_cpu.py, test_compute_sim3_gpu.py and tools/bench_compute_sim3_chain.py; nothing here touches the GPU."""
import numpy as np

import fuse_table_ref as R
import sim3_table_ref as Q

LIVE, BAD = Q.LIVE, Q.BAD
LEVEL_SIGMA2 = (Q.SCALE * Q.SCALE).astype("f4")                                  # mvLevelSigma2
INV_SIGMA2 = R.INV_SIGMA2                                                        # mvInvLevelSigma2
# mvnMaxError1 / 2 per level: 9.210 * mvLevelSigma2[level] pushed into a std::vector<size_t> (include/cslam/Sim3Solver.h:74-75)
MAX_ERR_LEVEL = np.trunc(9.210 * LEVEL_SIGMA2.astype("f8")).astype("f4")


def slots(pair, f1, f2):
    """The two map points of correspondences (f1, f2): the slots the keyframes hold at those features."""
    return np.asarray(pair["kf1"]["mp_id"])[np.asarray(f1, int)], np.asarray(pair["kf2"]["mp_id"])[np.asarray(f2, int)]


def solver_arrays(rows, pair, f1, f2, max_err_level1=MAX_ERR_LEVEL, max_err_level2=MAX_ERR_LEVEL):
    """mvX3Dc1 / mvX3Dc2 / mvnMaxError1 / 2 / mvnIndices1 of the constructor (:60-69) for correspondences that passed :32-59."""
    f1 = np.asarray(f1, int); f2 = np.asarray(f2, int)
    s1, s2 = slots(pair, f1, f2)
    pos = np.ascontiguousarray(rows["pos"], "f4")
    return dict(X1=Q.mat_point(pair["T1w"], pos[s1]).reshape(-1, 3), X2=Q.mat_point(pair["T2w"], pos[s2]).reshape(-1, 3),
                max_err1=np.asarray(max_err_level1, "f4")[pair["kf1"]["oct"][f1]], max_err2=np.asarray(max_err_level2, "f4")[pair["kf2"]["oct"][f2]],
                indices1=f1.astype("i4"))


def opt_arrays(rows, pair, f1, f2, inv_sigma2_1=INV_SIGMA2, inv_sigma2_2=INV_SIGMA2):
    """The six arrays of ccm_optimize_sim3 for correspondences that passed :922-935 (:938-989): the float camera-frame points, the
    undistorted keypoints and mvInvLevelSigma2[octave], widened to double."""
    f1 = np.asarray(f1, int); f2 = np.asarray(f2, int)
    s1, s2 = slots(pair, f1, f2)
    pos = np.ascontiguousarray(rows["pos"], "f4")
    k1, k2 = pair["kf1"], pair["kf2"]
    return dict(P1=Q.mat_point(pair["T1w"], pos[s1]).reshape(-1, 3).astype("f8"), P2=Q.mat_point(pair["T2w"], pos[s2]).reshape(-1, 3).astype("f8"),
                obs1=np.stack([k1["kx"][f1], k1["ky"][f1]], 1).astype("f4").astype("f8").reshape(-1, 2),
                obs2=np.stack([k2["kx"][f2], k2["ky"][f2]], 1).astype("f4").astype("f8").reshape(-1, 2),
                info1=np.asarray(inv_sigma2_1, "f4")[k1["oct"][f1]].astype("f8"), info2=np.asarray(inv_sigma2_2, "f4")[k2["oct"][f2]].astype("f8"))


def correspondences(rows, capacity, pair, match12):
    """The filter of src/Optimizer.cpp:920-957 on vpMatches1 after SearchBySim3, as (i1, i2) rows in ascending i1.  vpMatches1[i1] is
    the solver's inlier (matched12[i1] >= 0, held by kf2 at matched_idx2[i1]) or SearchBySim3's (match12[i1]); it becomes a
    correspondence when kf1's point at i1 and kf2's at i2 are set and not bad and i2 >= 0.  Any other match stays as it is."""
    fl = np.asarray(rows["flags"], np.uint8)
    id1 = np.asarray(pair["kf1"]["mp_id"]); id2 = np.asarray(pair["kf2"]["mp_id"])

    def good(s):
        return 0 <= s < capacity and (fl[s] & LIVE) != 0 and (fl[s] & BAD) == 0
    out = []
    for i1 in range(len(id1)):
        if pair["matched12"][i1] >= 0:
            i2 = int(pair["matched_idx2"][i1])
        elif match12[i1] >= 0:
            i2 = int(match12[i1])
        else:
            continue                                                             # :922
        if not (0 <= i2 < len(id2)):                                             # GetIndexInKeyFrame gave nothing
            continue
        if good(int(id1[i1])) and good(int(id2[i2])):                            # :933-935
            out.append((i1, i2))
    return np.array(out, "i4").reshape(-1, 2)


def chain_pair(scene, pair, match12, optimize):
    """Links 4 of the chain on one pair, from SearchBySim3's match12: the list, the arrays, OptimizeSim3 (optimize = the array entry
    point or the oracle: (sim3, fix_scale, K1, K2, P1, .., info2, th2) -> (sim3, inlier, nIn)) and vpMatches1[i1] = NULL as pruned."""
    corr = correspondences(scene["rows"], scene["capacity"], pair, match12)
    A = opt_arrays(scene["rows"], pair, corr[:, 0], corr[:, 1])
    K1 = np.asarray(pair["intr"], "f4").astype("f8"); K2 = np.asarray(pair.get("intr2", pair["intr"]), "f4").astype("f8")
    S, inl, nin = optimize(np.asarray(pair["sim3"], "f8"), int(pair.get("fix_scale", 0)), K1, K2, A["P1"], A["P2"], A["obs1"], A["obs2"], A["info1"], A["info2"],
                           float(pair.get("th2", 10.0)))
    pruned = np.zeros(len(pair["kf1"]["kx"]), np.uint8)
    pruned[corr[np.asarray(inl) == 0, 0]] = 1
    return dict(corr=corr, sim3=np.asarray(S, "f8").reshape(8), inlier=np.asarray(inl, np.uint8), n_inliers=int(nin), pruned=pruned)


def search_pair(scene, pair, th=7.5):
    """SearchBySim3 of the restatement alone: (n_found, match12)."""
    d1, d2 = Q.sim3_pair(scene, pair)
    found, m12, _, _ = Q.sim3_select(pair, d1, d2, th=th)
    return found, m12


def compute_sim3_sequential(solvers, chain_one, mInliersThres=20, mSolverIterations=5):
    """The loop of src/LoopFinder.cpp:284-346 as written: solvers[i].iterate(n) -> (Scm or None, bNoMore, vbInliers, nInliers);
    chain_one(i, Scm, vbInliers) -> dict with n_inliers, called where the reference calls SearchBySim3 and OptimizeSim3.  Returns
    (i, that dict, vbInliers) or None, and the list of chain calls made."""
    n = len(solvers)
    discarded = [False] * n
    n_candidates = n
    calls = []
    while n_candidates > 0:
        for i in range(n):
            if discarded[i]:
                continue
            Scm, no_more, vb, _ = solvers[i].iterate(mSolverIterations)
            if no_more:
                discarded[i] = True; n_candidates -= 1
            if Scm is not None:
                calls.append(i)
                res = chain_one(i, Scm, vb)
                if res["n_inliers"] >= mInliersThres:
                    return (i, res, vb), calls
    return None, calls


# ------------------------------------------------------------------------------------------------------------------ scenes
def quat_of(Rm):
    """Unit quaternion (x, y, z, w) of a rotation matrix with positive trace."""
    Rm = np.asarray(Rm, "f8")
    w = 0.5 * np.sqrt(1.0 + np.trace(Rm))
    return np.array([(Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w), w])


def true_sim3(pair, rng=None, rot=0.0, trans=0.0):
    """g2oS12 of a pair of Sim3Scene -- S12 = rows of [s12 R12 | t12] -- as qx, qy, qz, qw, tx, ty, tz, s, optionally off by a
    small rotation about a random axis and a translation (the estimate RANSAC hands over)."""
    S12 = np.asarray(pair["S12"], "f8"); s = float(np.cbrt(np.linalg.det(S12[:, :3])))
    q = quat_of(S12[:, :3] / s); t = S12[:, 3].copy()
    if rng is not None:
        q[:3] += rng.normal(0, rot, 3); q /= np.linalg.norm(q); t += rng.normal(0, trans, 3)
    return np.concatenate([q, t, [s]])


def true_pairs(scene, pair, px=1.5):
    """(i1, i2) where kf1's point at i1 is LIVE and lands within px of feature i2 of kf2, which holds a LIVE point of its own: the
    matches Sim3Scene.pair built, found from the geometry alone."""
    k1, k2 = pair["kf1"], pair["kf2"]
    if not len(k1["kx"]) or not len(k2["kx"]):
        return np.zeros((0, 2), "i4")
    d1 = Q.sim3_direction(scene["rows"], scene["capacity"], k1["mp_id"], np.zeros(len(k1["kx"]), bool), pair["T1w"], pair["S21"], pair["intr"], pair["bounds2"],
                          len(k2["kx"]))
    fl = scene["rows"]["flags"]

    def live(ids):
        inside = (ids >= 0) & (ids < scene["capacity"])
        return inside & ((fl[np.where(inside, ids, 0)] & LIVE) != 0)
    ok1 = live(k1["mp_id"]) & np.isin(d1["gate"], (Q.SEARCHED, Q.IS_BAD, Q.DISTANCE))
    ok2 = live(k2["mp_id"])
    out = []
    for i1 in np.flatnonzero(ok1):
        d = np.hypot(k2["kx"] - d1["u"][i1], k2["ky"] - d1["v"][i1])
        i2 = int(np.argmin(d))
        if d[i2] <= px and ok2[i2] and (d1["gate"][i1] != Q.IS_BAD):
            out.append((i1, i2))
    return np.array(out, "i4").reshape(-1, 2)


def gather_scene(n1, n2, seed, frac=1.0):
    """One table and one candidate pair of n1 x n2 synthetic features whose features (nearly) all hold a point."""
    sc = Q.Sim3Scene(seed)
    kf1 = sc.keyframe(R.synthetic_features(n1, seed), R.CAMERAS[0], frac=frac)
    sc.pair(kf1, n2, R.CAMERAS[1], 1.0, R.synthetic_features(n2, seed + 1), frac=frac)
    return sc.finish()


def live_features(scene, kf):
    ids = np.asarray(kf["mp_id"]); inside = (ids >= 0) & (ids < scene["capacity"])
    return np.flatnonzero(inside & ((scene["rows"]["flags"][np.where(inside, ids, 0)] & LIVE) != 0))


def pick_correspondences(scene, pair, n, rng, wrong=0.2):
    """n correspondences of a pair in ascending i1 with distinct i1: the true ones first, then wrong pairings of features that
    hold LIVE points (BAD ones included: the gathers do not look at BAD), a share `wrong` of the true ones swapped as well."""
    tp = true_pairs(scene, pair)
    l1, l2 = live_features(scene, pair["kf1"]), live_features(scene, pair["kf2"])
    assert len(l1) >= n and len(l2) >= 1, (len(l1), len(l2), n)
    take = tp[rng.permutation(len(tp))[:n]]
    rest = np.setdiff1d(l1, take[:, 0])
    extra = rng.permutation(rest)[:n - len(take)]
    c = np.concatenate([take, np.stack([extra, rng.choice(l2, len(extra))], 1)]).astype("i4").reshape(-1, 2)
    swap = rng.random(len(c)) < wrong
    c[swap, 1] = rng.choice(l2, int(swap.sum()))
    return c[np.argsort(c[:, 0])]


SOLVER_SIZES = (12, 64, 70)                       # kf1 of 90 features, kf2 of 80: below, exactly and past one mask word
OPT_SIZES = (0, 9, 10, 64, 65, 257)
CHAIN_N1 = (0, 63, 64, 65, 257)
CHAIN_SEED = 5


def chain_scene(seed=CHAIN_SEED):
    """The chain's scene: pairs with kf1 of 0, 63, 64, 65 and 257 features (pair 2 has the 64-feature keyframe on both sides under the
    identity, pair 3 has unequal K1 and K2), all on one table.  Per pair about a third of the true matches come in as the solver's inliers
    (matched12 / matched_idx2) together with wrong pairings, indices outside kf2 and -- in the largest pair -- one whose point is
    BAD; sim3 is the true S12 slightly off; th2 10 / 20 and fix_scale mixed."""
    rng = np.random.default_rng(seed)
    sc = Q.Sim3Scene(seed)
    feats = {n: R.synthetic_features(max(n, 1), seed + n) for n in CHAIN_N1}
    plan = []
    for j, n1 in enumerate(CHAIN_N1):
        kf1 = sc.keyframe(R.cut(feats[n1], slice(0, n1)), R.CAMERAS[j % 4], frac=0.95 if n1 != 63 else 0.22)
        if n1 == 64:
            p = sc.pair(kf1, n1, None, 1.0, None, kf2=kf1)
            I = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype("f4")
            p["S12"] = I; p["S21"] = I.copy()
        else:
            n2 = max(n1 - 1, 1) if n1 else 40
            p = sc.pair(kf1, n2, R.CAMERAS[(j + 1) % 4], 1.0, R.synthetic_features(n2, seed + 100 + n1), frac=0.95)
        plan.append(p)
    scene = sc.finish()
    for j, p in enumerate(plan):
        n1, n2 = len(p["kf1"]["kx"]), len(p["kf2"]["kx"])
        m12 = np.full(n1, -1, "i4"); mi2 = np.full(n1, -1, "i4")
        tp = true_pairs(scene, p) if p["kf1"] is not p["kf2"] else np.stack([live_features(scene, p["kf1"])] * 2, 1)
        mark = tp[rng.random(len(tp)) < 0.35]
        m12[mark[:, 0]] = p["kf2"]["mp_id"][mark[:, 1]]; mi2[mark[:, 0]] = mark[:, 1]
        free = np.setdiff1d(live_features(scene, p["kf1"]), mark[:, 0])
        l2 = live_features(scene, p["kf2"])
        if len(free) >= 6 and len(l2):
            w = rng.permutation(free)[:6]
            m12[w] = 7
            mi2[w[:3]] = rng.choice(l2, 3)                                   # wrong pairings: correspondences the optimiser prunes
            mi2[w[3:]] = (-1, n2, n2 + 5)                                    # no index in kf2: left alone
        if n1 == 257:
            i1 = int(mark[0, 0])                                             # a solver inlier whose point has gone bad since
            scene["rows"]["flags"][p["kf1"]["mp_id"][i1]] |= BAD
            p["bad_i1"] = i1
        p["matched12"] = m12; p["matched_idx2"] = mi2
        p["sim3"] = true_sim3(p, rng, rot=0.002, trans=0.01)
        p["fix_scale"] = j % 2; p["th2"] = 10.0 if j % 2 == 0 else 20.0
        if n1 == 65:
            p["intr2"] = (452.0, 455.0, 360.0, 250.0)
    return scene
