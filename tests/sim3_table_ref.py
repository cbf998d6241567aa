"""numpy restatement of the projections and gates of ccm_search_by_sim3_table_frames and ccm_search_by_projection_table_frames
(include/ccm_hot.h), written from the reference's text: ORBmatcher::SearchBySim3 (src/ORBmatcher.cpp:1154-1211, :1250-1291),
SearchByProjection(pKF, Scw, ...) (:324-378) and MapPoint::PredictScale (src/MapPoint.cpp:837-852), in float32 storage with float64
sums in the stated order; and the scenes the tests use.  The selections come from tests/window_matcher_ref.py.  Shared by
test_sim3_table_cpu.py, test_sim3_table_gpu.py, test_loop_projection_table_gpu.py and tools/bench_compute_sim3_table.py; nothing here
touches the GPU."""
import numpy as np

import fuse_table_ref as R
import search_local_points_ref as S
import window_matcher_ref as W

F = np.float32
LIVE, BAD, HAS_OBS = S.LIVE, S.BAD, S.HAS_OBS
SEARCHED, NO_POINT, MATCHED, IS_BAD, BEHIND, OUTSIDE, DISTANCE, EMPTY_KF = range(8)        # CCM_SG_*
LG_SEARCHED, LG_SKIPPED, LG_ALREADY_FOUND, LG_BEHIND, LG_OUTSIDE, LG_DISTANCE, LG_ANGLE, LG_EMPTY_KF = range(8)   # CCM_LG_*
INTR, BOUNDS, SCALE, LOG_SF, N_LEVELS = S.INTR, S.BOUNDS, S.SCALE, S.LOG_SF, S.N_LEVELS
SHIFT2 = int(np.ceil(np.log(2.0) / np.log(1.2)))                 # levels that a factor 2 in distance moves PredictScale: 4


def mat_point(M, P):
    """Row-major [3][4] float32 M times (P, 1) per row of P [n][3]: the sum in double in the order written, stored as float."""
    Md = np.asarray(M, "f4").reshape(3, 4).astype("f8"); Pd = np.asarray(P, "f4").astype("f8")
    return np.stack([((Md[r, 0] * Pd[:, 0] + Md[r, 1] * Pd[:, 1]) + Md[r, 2] * Pd[:, 2]) + Md[r, 3] for r in range(3)], 1).astype("f4")


def predict_level(max_dist, dist, log_sf=LOG_SF, n_levels=N_LEVELS):
    """PredictScale: ceil(float(log(double(max_dist / dist))) / log_sf) clamped, a NaN gives 0.  Returns (level, ambiguous): ambiguous
    where one ulp more or less on the logarithm changes the level."""
    with np.errstate(all="ignore"):
        lg = np.log((np.asarray(max_dist, "f4") / np.asarray(dist, "f4")).astype("f8")).astype("f4")

        def lvl(l):
            c = np.ceil(l / F(log_sf))
            return np.where(~(c >= 0), 0, np.where(c >= n_levels, n_levels - 1, c)).astype("i4")
        level = lvl(lg)
        amb = (lvl(np.nextafter(lg, F(np.inf))) != level) | (lvl(np.nextafter(lg, F(-np.inf))) != level)
    return level, amb


def sim3_direction(rows, capacity, mp_id, marked, Tsw, Sts, intr, bounds_t, n_target, log_sf=LOG_SF, n_levels=N_LEVELS):
    """One direction of SearchBySim3 for the features of the source keyframe: mp_id [n] table slots, marked [n] = vbAlreadyMatched,
    Tsw = the source's [R | t], Sts = [sR | t] into the target, intr = pKF1's intrinsics, bounds_t / n_target = the target's image
    bounds and feature count.  Returns dict(gate [n] CCM_SG_*, u, v, level, dist, ambiguous, desc [n][32]); u / v are 0 where the
    feature did not reach the projection and level is 0 where it did not reach PredictScale, as on the device."""
    ids = np.asarray(mp_id, "i4").reshape(-1); n = len(ids)
    inside = (ids >= 0) & (ids < capacity)
    s = np.where(inside, ids, 0)
    fl = np.where(inside, np.asarray(rows["flags"], np.uint8)[s], 0).astype(np.uint8)
    P = np.ascontiguousarray(rows["pos"], "f4")[s]
    mn = np.ascontiguousarray(rows["min_dist"], "f4")[s]; mx = np.ascontiguousarray(rows["max_dist"], "f4")[s]
    fx, fy, cx, cy = [F(v) for v in intr]; x0, x1, y0, y1 = [F(v) for v in bounds_t]
    with np.errstate(all="ignore"):
        Ps = mat_point(Tsw, P)                                   # :1181 / :1261
        Pt = mat_point(Sts, Ps)                                  # :1182 / :1262
        invz = F(1.0) / Pt[:, 2]
        x = Pt[:, 0] * invz; y = Pt[:, 1] * invz
        u = fx * x + cx; v = fy * y + cy
        Pd = Pt.astype("f8")
        dist = np.sqrt((Pd[:, 0] * Pd[:, 0] + Pd[:, 1] * Pd[:, 1]) + Pd[:, 2] * Pd[:, 2]).astype("f4")      # cv::norm
        level, amb = predict_level(mx, dist, log_sf, n_levels)
        gate = np.full(n, SEARCHED if n_target > 0 else EMPTY_KF, "i4")
        for k, rej in ((DISTANCE, (dist < F(0.8) * mn) | (dist > F(1.2) * mx)), (OUTSIDE, ~((u >= x0) & (u < x1) & (v >= y0) & (v < y1))),
                       (BEHIND, Pt[:, 2] < 0), (IS_BAD, (fl & BAD) != 0), (MATCHED, np.asarray(marked, bool)), (NO_POINT, (fl & LIVE) == 0)):
            gate[rej] = k                                        # the earliest test wins: assigned last
    proj = (gate == SEARCHED) | (gate >= OUTSIDE)
    done = (gate == SEARCHED) | (gate == EMPTY_KF)
    return dict(gate=gate, u=np.where(proj, u, F(0)).astype("f4"), v=np.where(proj, v, F(0)).astype("f4"), level=np.where(done, level, 0).astype("i4"),
                dist=dist, ambiguous=amb & done, desc=np.asarray(rows["desc"], np.uint8)[s])


def marks(pair):
    """vbAlreadyMatched1 / 2 of a pair (:1154-1164): an index outside [0, N2) is ignored."""
    m12 = np.asarray(pair["matched12"], "i4"); i2 = np.asarray(pair["matched_idx2"], "i4")
    n2 = len(pair["kf2"]["kx"])
    a1 = m12 >= 0
    a2 = np.zeros(n2, bool)
    ok = a1 & (i2 >= 0) & (i2 < n2)
    a2[i2[ok]] = True
    return a1, a2


def sim3_pair(scene, pair):
    """Both directions of one pair.  Only pair['intr'] -- pKF1's intrinsics -- is used, for both directions (:1127-1130, :1272); a
    pair may carry 'intr2' (pKF2's own) to show that it is not."""
    a1, a2 = marks(pair)
    k1, k2 = pair["kf1"], pair["kf2"]
    d1 = sim3_direction(scene["rows"], scene["capacity"], k1["mp_id"], a1, pair["T1w"], pair["S21"], pair["intr"], pair["bounds2"], len(k2["kx"]))
    d2 = sim3_direction(scene["rows"], scene["capacity"], k2["mp_id"], a2, pair["T2w"], pair["S12"], pair["intr"], pair["bounds1"], len(k1["kx"]))
    return d1, d2


def grid(kf, bounds=BOUNDS):
    return W.Grid(kf["kx"], kf["ky"], kf["oct"], kf["desc"], min_x=bounds[0], max_x=bounds[1], min_y=bounds[2], max_y=bounds[3])


def sim3_select(pair, d1, d2, level1=None, level2=None, th=7.5):
    """The two selection passes and the agreement check on the restatement's projections (window_matcher_ref).  Returns
    (n_found, match12, sel1, sel2)."""
    g1, g2 = grid(pair["kf1"], pair["kf1"].get("bounds", BOUNDS)), grid(pair["kf2"], pair["kf2"].get("bounds", BOUNDS))
    l1 = d1["level"] if level1 is None else level1; l2 = d2["level"] if level2 is None else level2
    v1 = d1["gate"] == SEARCHED; v2 = d2["gate"] == SEARCHED
    sel1, _ = W.fuse_select(g2, SCALE, None, v1, d1["u"], d1["v"], l1, d1["desc"], th, False, W.TH_HIGH)
    sel2, _ = W.fuse_select(g1, SCALE, None, v2, d2["u"], d2["v"], l2, d2["desc"], th, False, W.TH_HIGH)
    found, m12 = W.search_by_sim3(g1, SCALE, g2, SCALE, v1, d1["u"], d1["v"], l1, d1["desc"], v2, d2["u"], d2["v"], l2, d2["desc"], th)
    return found, m12, sel1, sel2


# ------------------------------------------------------------------------------------------------------------------ Sim3 scenes
def sim3_of(s12, rotvec=(0.02, -0.03, 0.015), t=(0.3, -0.2, 0.25)):
    """S12 = rows of [s12 R12 | t12] and S21 = rows of [(1 / s12) R12^T | -sR21 t12] (:1141-1143), float32."""
    T, _ = S.camera(rotvec, t)
    R12 = T[:, :3].astype("f8"); t12 = T[:, 3].astype("f8")
    sR12 = s12 * R12; sR21 = (1.0 / s12) * R12.T; t21 = -sR21 @ t12
    return np.concatenate([sR12, t12[:, None]], 1).astype("f4"), np.concatenate([sR21, t21[:, None]], 1).astype("f4")


class Sim3Scene:
    """A table and candidate pairs on it.  keyframe(): a keyframe whose `frac` of features hold a point made for them; pair(): a second
    keyframe whose features are the projections of the first one's points through S21 T1w (plus distractors), with points of its
    own that project back onto the first keyframe's features; finish(): the rows in permuted slots, a twentieth BAD, a twentieth not
    LIVE, two ids per keyframe outside the table."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed); self.seed = seed
        self.parts = []; self.n_rows = 0; self.kfs = []; self.pairs = []

    def _rows(self, rows):
        first = self.n_rows
        n = len(rows["flags"])
        self.parts.append(rows); self.n_rows += n
        return np.arange(first, first + n, dtype="i4")

    def keyframe(self, feat, cam, frac=0.6, intr=INTR):
        n = len(feat["kx"])
        ids = np.full(n, -1, "i4")
        hold = np.flatnonzero(self.rng.random(n) < frac)
        if len(hold):
            ids[hold] = self._rows(S.matchable_points(feat["kx"][hold], feat["ky"][hold], feat["oct"][hold], feat["desc"][hold], *cam,
                                                      seed=self.seed + 17 * len(self.kfs), intr=intr))
        kf = dict(R.cut(feat, slice(None)), Tcw=cam[0], Ow=cam[1], mp_id=ids)
        self.kfs.append(kf)
        return kf

    def pair(self, kf1, n2, cam2, s12, distract, frac=0.6, n_marked=0, intr=INTR, bounds1=BOUNDS, bounds2=BOUNDS, kf2=None):
        """distract: features (dict) that fill the second keyframe up to n2.  kf2: use this keyframe (e.g. kf1 itself) instead."""
        rng = self.rng
        S12, S21 = sim3_of(s12)
        n1 = len(kf1["kx"])
        if kf2 is None:
            pool = np.concatenate(self.parts_dict("pos")) if self.parts else np.zeros((0, 3), "f4")
            mxd = np.concatenate(self.parts_dict("max_dist")) if self.parts else np.zeros(0, "f4")
            hold = np.flatnonzero(kf1["mp_id"] >= 0)
            P1 = pool[kf1["mp_id"][hold]].astype("f8")
            T1 = np.asarray(kf1["Tcw"], "f8"); Sd = S21.astype("f8"); T2 = np.asarray(cam2[0], "f8")
            Pc1 = P1 @ T1[:, :3].T + T1[:, 3]; Pc2 = Pc1 @ Sd[:, :3].T + Sd[:, 3]
            with np.errstate(all="ignore"):
                u = intr[0] * Pc2[:, 0] / Pc2[:, 2] + intr[2]; v = intr[1] * Pc2[:, 1] / Pc2[:, 2] + intr[3]
                o2 = np.clip(np.ceil(np.log(mxd[kf1["mp_id"][hold]] / np.linalg.norm(Pc2, axis=1)) / np.log(1.2)), 0, 7)
            ok = (Pc2[:, 2] > 0) & (u >= bounds2[0] + 1) & (u < bounds2[1] - 1) & (v >= bounds2[2] + 1) & (v < bounds2[3] - 1)
            src = hold[ok][:n2]                                               # the features of kf1 that reappear in kf2
            m = len(src)
            flips = np.packbits(rng.random((m, 256)) < 0.03, axis=1, bitorder="little")
            nd = n2 - m
            feat2 = dict(kx=np.concatenate([u[ok][:m] + rng.normal(0, 0.3, m), distract["kx"][:nd]]).astype("f4"),
                         ky=np.concatenate([v[ok][:m] + rng.normal(0, 0.3, m), distract["ky"][:nd]]).astype("f4"),
                         oct=np.concatenate([o2[ok][:m], distract["oct"][:nd]]).astype("i4"),
                         desc=np.concatenate([kf1["desc"][src] ^ flips, distract["desc"][:nd]]))
            assert len(feat2["kx"]) == n2, "not enough distractors"
            ids2 = np.full(n2, -1, "i4")
            own = np.flatnonzero(rng.random(m) < frac)                         # kf2's own points: T2w P2 = Pc2, so S12 T2w P2 = Pc1
            if len(own):
                Pw2 = (Pc2[ok][:m][own] - T2[:, 3]) @ T2[:, :3]
                d1 = np.linalg.norm(Pc1[ok][:m][own], axis=1)
                mx = d1 * 1.2 ** (kf1["oct"][src][own].astype("f8") - 0.5)
                fl = np.packbits(rng.random((len(own), 256)) < 0.05, axis=1, bitorder="little")
                ids2[own] = self._rows(dict(pos=Pw2.astype("f4"), normal=np.zeros((len(own), 3), "f4"), min_dist=(mx / 1.2 ** 7).astype("f4"),
                                            max_dist=mx.astype("f4"), desc=kf1["desc"][src][own] ^ fl, flags=np.full(len(own), LIVE | HAS_OBS, np.uint8)))
            far = m + np.flatnonzero(rng.random(nd) < frac)                    # distractor features hold random points
            if len(far):
                ids2[far] = self._rows(S.random_points(len(far), self.seed + 31 * len(self.pairs) + 5))
            order = rng.permutation(n2)
            kf2 = dict(R.cut(feat2, order), Tcw=cam2[0], Ow=cam2[1], mp_id=ids2[order])
            self.kfs.append(kf2)
        n2 = len(kf2["kx"])
        m12 = np.full(n1, -1, "i4"); mi2 = np.full(n1, -1, "i4")
        if n_marked and n1:
            who = rng.permutation(n1)[:n_marked]
            m12[who] = rng.integers(0, 1 << 20, len(who))                      # any slot: only its sign is read
            mi2[who] = np.resize(np.array([0, n2 // 2, n2 - 1, -1, -7, n2, n2 + 5, 3], "i4"), len(who))
            if len(who) > 8 and n2:
                mi2[who[8:]] = rng.integers(0, n2, len(who) - 8)
            mi2[rng.permutation(n1)[:3]] = 1                                   # an index without a point in matched12 marks nothing
        p = dict(kf1=kf1, kf2=kf2, T1w=kf1["Tcw"], T2w=kf2["Tcw"], S12=S12, S21=S21, intr=intr, bounds1=bounds1, bounds2=bounds2,
                 matched12=m12, matched_idx2=mi2, s12=s12)
        self.pairs.append(p)
        return p

    def parts_dict(self, col):
        return [np.asarray(p[col]) for p in self.parts]

    def finish(self, spare=7):
        rng = self.rng
        n = self.n_rows; cap = n + spare
        pool = S.concat(*self.parts) if self.parts else {c: np.zeros((0,) + sh, dt) for c, sh, dt in
                                                         (("pos", (3,), "f4"), ("normal", (3,), "f4"), ("min_dist", (), "f4"), ("max_dist", (), "f4"),
                                                          ("desc", (32,), np.uint8), ("flags", (), np.uint8))}
        perm = rng.permutation(cap)[:n].astype("i4")
        rows = dict(pos=np.zeros((cap, 3), "f4"), normal=np.zeros((cap, 3), "f4"), min_dist=np.zeros(cap, "f4"), max_dist=np.zeros(cap, "f4"),
                    desc=np.zeros((cap, 32), np.uint8), flags=np.zeros(cap, np.uint8))
        for c in R.COLS:
            rows[c][perm] = pool[c]
        kind = rng.random(n)
        rows["flags"][perm[kind < 0.05]] |= BAD
        rows["flags"][perm[(kind >= 0.05) & (kind < 0.10)]] &= ~np.uint8(LIVE)
        for kf in self.kfs:
            ids = kf["mp_id"]
            ids[ids >= 0] = perm[ids[ids >= 0]]
            free = np.flatnonzero(ids < 0)
            if len(free) >= 2:
                ids[free[0]] = cap; ids[free[1]] = 1 << 30                    # ids outside the table: NO_POINT
        return dict(rows=rows, capacity=cap, pairs=self.pairs, kfs=self.kfs)


def cuts(feat, n, seed):
    """n features of `feat` (sorted random indices)."""
    rng = np.random.default_rng(seed)
    return R.cut(feat, np.sort(rng.choice(len(feat["kx"]), n, replace=False)))


SIM3_SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
SIM3_CASES = [(n1, n2, 1 + (i + j) % 3) for i, n1 in enumerate(SIM3_SIZES) for j, n2 in enumerate(SIM3_SIZES) if (i + 2 * j) % 4 == 0 or n1 == n2]
SIM3_SEED = 11            # with this seed the restatement alone meets the scene conditions of test_sim3_table_cpu.py


def sim3_scene(feat, n1, n2, n_pairs, seed=SIM3_SEED, s12=(1.0, 2.0, 1.0)):
    """n_pairs candidate pairs on one table: kf1 of n1 features (shared by pairs 0 and 1 where there are two), kf2 of n2 each."""
    sc = Sim3Scene(1000 * n1 + 10 * n2 + n_pairs + seed)
    kf1 = None
    for p in range(n_pairs):
        if p != 1:
            kf1 = sc.keyframe(cuts(feat, n1, seed + 3 * p + n1), R.CAMERAS[p % 4])
        sc.pair(kf1, n2, R.CAMERAS[(p + 1) % 4], s12[(p + n1 + n2) % len(s12)] if n_pairs > 1 else s12[0],
                cuts(feat, max(n2, 1), seed + 50 + p + n2), n_marked=min(n1, 9 if p == 0 else 0))
    return sc.finish()


def big_sim3_scene(feat_of, n_pairs, n=1000):
    """n_pairs pairs of n x n features, about 60 % of them holding points (the benchmark's size).  feat_of(k) = features of keyframe k."""
    sc = Sim3Scene(77 + n_pairs)
    for p in range(n_pairs):
        kf1 = sc.keyframe(feat_of(2 * p), R.CAMERAS[p % 4])
        sc.pair(kf1, n, R.CAMERAS[(p + 1) % 4], 1.0, feat_of(2 * p + 1), n_marked=20)
    return sc.finish()


# ------------------------------------------------------------------------------------------------------------------ loop projection
def loop_views(scene):
    """The restatement of SearchByProjection(pKF, Scw, ...) up to the queries for every view of a Fuse scene (fuse_table_ref.make_scene)
    that also carries matched_slot per keyframe: the gates of :335-375 are Fuse's second overload's with spAlreadyFound in the place of
    IsInKeyFrame.  Returns dict(gate, u, v, level, ambiguous, observed), each [K][n]."""
    slots = scene["slots"]
    out = []
    for kf in scene["kfs"]:
        ms = np.asarray(kf["matched_slot"], "i4")
        found = np.isin(slots, ms[ms >= 0])
        g = R.gates(scene["rows"], slots, kf["Tcw"], kf["Ow"], kf.get("intr", INTR), kf.get("bounds", BOUNDS), held=found, n_feat=len(kf["kx"]))
        g["observed"] = R.held_by(kf["mp_id"], slots).astype(np.uint8)
        out.append(g)
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


def loop_accept(scene, g, level=None, th=10.0):
    """The acceptance of every view in list order (window_matcher_ref.search_by_projection_sim3) and what it does to matched_slot.
    Returns (n_matches [K], best_idx [K][n], matched_slot per view)."""
    slots = scene["slots"]
    desc = scene["rows"]["desc"][slots]
    level = g["level"] if level is None else level
    nm, bi, ms_out = [], [], []
    for k, kf in enumerate(scene["kfs"]):
        ms = np.asarray(kf["matched_slot"], "i4").copy()
        n, b, mt = W.search_by_projection_sim3(grid(kf, kf.get("bounds", BOUNDS)), SCALE, g["gate"][k] == LG_SEARCHED, g["u"][k], g["v"][k], level[k], desc,
                                               g["observed"][k], ms >= 0, th)
        new = np.flatnonzero((b >= 0) & (g["observed"][k] == 0))
        assert (ms[b[new]] < 0).all() and len(set(b[new].tolist())) == len(new) and (mt.astype(bool) == ((ms >= 0) | np.isin(np.arange(len(ms)), b[new]))).all()
        ms[b[new]] = slots[new]
        nm.append(n); bi.append(b); ms_out.append(ms)
    return np.array(nm, "i4"), np.stack(bi) if bi else np.zeros((0, len(slots)), "i4"), ms_out


LOOP_SEED = 5


def loop_scene(feat, n_points, n_kf, n_feat=64, seed=LOOP_SEED, n_hold=8):
    """A Fuse scene (n_kf keyframes of n_feat features cut from `feat`, n_points points) with vpMatched per keyframe: six features
    matched on entry -- three to listed slots (ALREADY_FOUND), two to slots outside the list, one to a slot outside the table."""
    rng = np.random.default_rng(1000 * n_points + n_kf + seed)
    cs = [R.cut(feat, np.sort(rng.choice(len(feat["kx"]), n_feat, replace=False))) for _ in range(n_kf)]
    sc = R.make_scene(cs, n_points, n_feat, n_hold, seed=n_points + n_kf + seed)
    unlisted = np.setdiff1d(np.arange(sc["capacity"]), sc["slots"])
    for kf in sc["kfs"]:
        ms = np.full(len(kf["kx"]), -1, "i4")
        if len(ms) >= 16:
            who = rng.permutation(len(ms))[:6]
            ms[who[:3]] = sc["slots"][rng.permutation(n_points)[:3]] if n_points >= 3 else unlisted[0]
            ms[who[3:5]] = unlisted[:2]; ms[who[5]] = sc["capacity"] + 3
        kf["matched_slot"] = ms
    return sc


def big_loop_scene():
    """One keyframe of 1,000 synthetic features x 4,000 loop points (the benchmark's size)."""
    sc = R.make_scene([R.synthetic_features(1000, 60)], 4000, 700, 100, seed=21)
    sc["kfs"][0]["matched_slot"] = np.full(1000, -1, "i4")
    sc["kfs"][0]["matched_slot"][::50] = sc["slots"][:20]
    return sc


# Two points whose windows share their nearest feature (distances 2 | 49 for the first point, 1 | 52 for the second)
HAND_SHARED = ([(300.0, 200.0, 2, 1), (303.0, 200.0, 2, 52)], [(300.5, 200.0, 2, 3), (301.0, 200.0, 2, 0)])


# Seventy octave-2 features on a 1-px lattice, 10 x 7, around (300, 200): every one lies inside the window of either point of
# HAND_SHARED at th = 10 (radius 10 * 1.2^2 = 14.4 px), so their lists hold 70 > 64 candidates.  Feature 37 is at distance 7 | 10 from
# the two points, the others at 60 or more.
HAND_CROWDED = [(296.0 + i % 10, 197.0 + i // 10, 2, 10 if i == 37 else 63 + i) for i in range(70)]


def retry_scene():
    """The points of HAND_SHARED seen by two views of one table: view 0 is HAND_SHARED's (short lists, one match), view 1 the crowded
    one, whose lists overflow the first capacity of the device route so that every view repeats."""
    sc = hand_scene(*HAND_SHARED)
    sc["kfs"].append(hand_scene(HAND_CROWDED, HAND_SHARED[1])["kfs"][0])
    return sc


def longest_lists(scene, th=10.0):
    """Per view, the length of the longest GetFeaturesInArea list among the searched points (window_matcher_ref.features_in_area)."""
    g = loop_views(scene)
    out = []
    for k, kf in enumerate(scene["kfs"]):
        G = grid(kf, kf.get("bounds", BOUNDS))
        out.append(max([len(W.features_in_area(G, g["u"][k][j], g["v"][k][j], F(th) * F(SCALE[g["level"][k][j]])))
                        for j in np.flatnonzero(g["gate"][k] == LG_SEARCHED)], default=0))
    return out


def hand_scene(features, points, matched_slot=None, held=()):
    """Hand-built order cases under the identity camera.  features: (x, y, octave, bits) per feature; points: (x, y, octave, bits) per
    point, projected exactly onto (x, y) at depth 4 and predicting `octave`; bits = how many leading bits of the all-zero descriptor
    are set.  held: (feature, point) pairs -- the keyframe observes the point there.  Slot j = point j."""
    def desc(bits):
        d = np.zeros(256, np.uint8); d[:bits] = 1
        return np.packbits(d, bitorder="little")
    nf, npt = len(features), len(points)
    kf = dict(kx=np.array([f[0] for f in features], "f4"), ky=np.array([f[1] for f in features], "f4"), oct=np.array([f[2] for f in features], "i4"),
              desc=np.stack([desc(f[3]) for f in features]) if nf else np.zeros((0, 32), np.uint8), Tcw=S.IDENTITY[0], Ow=S.IDENTITY[1],
              mp_id=np.full(nf, -1, "i4"), matched_slot=np.full(nf, -1, "i4") if matched_slot is None else np.asarray(matched_slot, "i4"))
    for f, j in held:
        kf["mp_id"][f] = j
    z = 4.0
    pos = np.array([[(p[0] - INTR[2]) / INTR[0] * z, (p[1] - INTR[3]) / INTR[1] * z, z] for p in points], "f8").reshape(npt, 3)
    d = np.linalg.norm(pos, axis=1)
    mx = d * 1.2 ** (np.array([p[2] for p in points], "f8") - 0.5)
    rows = dict(pos=pos.astype("f4"), normal=(pos / d[:, None]).astype("f4"), min_dist=(mx / 1.2 ** 7).astype("f4"), max_dist=mx.astype("f4"),
                desc=np.stack([desc(p[3]) for p in points]), flags=np.full(npt, LIVE | HAS_OBS, np.uint8))
    return dict(kfs=[kf], rows=rows, slots=np.arange(npt, dtype="i4"), capacity=npt)
