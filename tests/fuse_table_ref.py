"""numpy restatement of the gates of ccm_fuse_select_table_frames (include/ccm_hot.h): the projection and the tests of
ORBmatcher::Fuse, both overloads (src/ORBmatcher.cpp:870-920, :1018-1071), and MapPoint::PredictScale (src/MapPoint.cpp:837-852) in
float32 storage with float64 sums, a brute-force restatement of the selection (for counting only), and the scenes the tests use.
Shared by test_fuse_table_cpu.py, test_fuse_table_gpu.py and tools/bench_fuse_table.py; nothing here touches the GPU."""
import numpy as np

import search_local_points_ref as S

F = np.float32
LIVE, BAD, HAS_OBS = S.LIVE, S.BAD, S.HAS_OBS
SEARCHED, SKIPPED, IN_KEYFRAME, BEHIND, OUTSIDE, DISTANCE, ANGLE, EMPTY_KF = range(8)      # CCM_FG_*
INTR, BOUNDS, SCALE, LOG_SF, N_LEVELS = S.INTR, S.BOUNDS, S.SCALE, S.LOG_SF, S.N_LEVELS
INV_SIGMA2 = (F(1.0) / (SCALE * SCALE)).astype("f4")             # mvInvLevelSigma2
COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")


def gates(rows, slots, Tcw, Ow, intr=INTR, bounds=BOUNDS, held=None, skip=None, n_feat=1, log_sf=LOG_SF, n_levels=N_LEVELS):
    """The gates of one keyframe for the points rows[slots].  held [n] = the keyframe already holds the point, skip [n] = the
    caller's skip flags, n_feat = the keyframe's feature count.  Returns dict(gate [n] CCM_FG_*, u, v, level, dist, ambiguous);
    u / v are 0 where the pair did not reach the projection and level is 0 where it did not reach PredictScale, as on the device."""
    slots = np.asarray(slots, "i4").reshape(-1)
    n = len(slots)
    P = np.ascontiguousarray(rows["pos"], "f4")[slots]; Pn = np.ascontiguousarray(rows["normal"], "f4")[slots]
    mn = np.ascontiguousarray(rows["min_dist"], "f4")[slots]; mx = np.ascontiguousarray(rows["max_dist"], "f4")[slots]
    fl = np.asarray(rows["flags"], np.uint8)[slots]
    T = np.asarray(Tcw, "f4").reshape(3, 4); Ow = np.asarray(Ow, "f4").reshape(3)
    fx, fy, cx, cy = [F(v) for v in intr]; x0, x1, y0, y1 = [F(v) for v in bounds]
    held = np.zeros(n, bool) if held is None else np.asarray(held, bool)
    skip = np.zeros(n, bool) if skip is None else np.asarray(skip, bool)
    Pd = P.astype("f8"); Td = T.astype("f8")
    with np.errstate(all="ignore"):
        Pc = np.stack([((Td[r, 0] * Pd[:, 0] + Td[r, 1] * Pd[:, 1]) + Td[r, 2] * Pd[:, 2]) + Td[r, 3] for r in range(3)], 1).astype("f4")
        invz = F(1.0) / Pc[:, 2]
        x = Pc[:, 0] * invz; y = Pc[:, 1] * invz                 # :890-892: the division first ...
        u = fx * x + cx; v = fy * y + cy                         # :894-895: ... then the intrinsics, every operation rounded to float
        PO = P - Ow[None, :]
        POd = PO.astype("f8")
        dist = np.sqrt((POd[:, 0] * POd[:, 0] + POd[:, 1] * POd[:, 1]) + POd[:, 2] * POd[:, 2]).astype("f4")
        Nd = Pn.astype("f8")
        dot = (POd[:, 0] * Nd[:, 0] + POd[:, 1] * Nd[:, 1]) + POd[:, 2] * Nd[:, 2]
        lg = np.log((mx / dist).astype("f8")).astype("f4")

        def lvl(l):
            c = np.ceil(l / F(log_sf))
            return np.where(~(c >= 0), 0, np.where(c >= n_levels, n_levels - 1, c)).astype("i4")
        level = lvl(lg)
        amb = (lvl(np.nextafter(lg, F(np.inf))) != level) | (lvl(np.nextafter(lg, F(-np.inf))) != level)
        gate = np.full(n, SEARCHED if n_feat > 0 else EMPTY_KF, "i4")
        for k, rej in ((ANGLE, dot < 0.5 * dist.astype("f8")), (DISTANCE, (dist < F(0.8) * mn) | (dist > F(1.2) * mx)),
                       (OUTSIDE, ~((u >= x0) & (u < x1) & (v >= y0) & (v < y1))), (BEHIND, Pc[:, 2] < 0), (IN_KEYFRAME, held),
                       (SKIPPED, skip | ((fl & LIVE) == 0) | ((fl & BAD) != 0))):
            gate[rej] = k                                        # the earliest test wins: assigned last
    proj = (gate == SEARCHED) | (gate >= OUTSIDE)
    done = (gate == SEARCHED) | (gate == EMPTY_KF)
    return dict(gate=gate, u=np.where(proj, u, F(0)).astype("f4"), v=np.where(proj, v, F(0)).astype("f4"), level=np.where(done, level, 0).astype("i4"),
                dist=dist, ambiguous=amb & done)


def held_by(mp_id, slots):
    """held [n]: some feature of the keyframe holds slots[j] (an id that names no listed slot is ignored)."""
    return np.isin(np.asarray(slots, "i4"), np.asarray(mp_id, "i4"))


def fuse_gates(scene, skip=None):
    """gates() for every keyframe of a scene, stacked [K][n]."""
    out = [gates(scene["rows"], scene["slots"], kf["Tcw"], kf["Ow"], kf.get("intr", INTR), kf.get("bounds", BOUNDS),
                 held=held_by(kf["mp_id"], scene["slots"]), skip=skip, n_feat=len(kf["kx"])) for kf in scene["kfs"]]
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


def select(kf, u, v, level, desc, th, chi2_check, scale=SCALE, inv_sigma2=INV_SIGMA2):
    """Smallest descriptor distance among the keyframe's features of level - 1 .. level with |dx| < r and |dy| < r (and, with
    chi2_check, a reprojection error within 5.99), per query; 256 where there is none.  For counting: which of equal distances
    wins is not restated here, the GPU tests take the indices from the array entry point."""
    kx = np.asarray(kf["kx"], "f4"); ky = np.asarray(kf["ky"], "f4"); oc = np.asarray(kf["oct"], "i4"); fd = np.asarray(kf["desc"], np.uint8)
    best = np.full(len(u), 256, "i4")
    for q in range(len(u)):
        r = F(th) * scale[level[q]]
        ex = F(u[q]) - kx; ey = F(v[q]) - ky
        ok = (np.abs(ex) < r) & (np.abs(ey) < r) & (oc >= level[q] - 1) & (oc <= level[q])
        if chi2_check:
            ok &= ~(((ex * ex + ey * ey) * inv_sigma2[np.clip(oc, 0, len(inv_sigma2) - 1)]).astype("f8") > 5.99)
        if ok.any():
            best[q] = np.unpackbits(fd[ok] ^ np.asarray(desc[q], np.uint8)[None, :], axis=1).sum(1).min()
    return best


# ------------------------------------------------------------------------------------------------------------------ scenes
CAMERAS = [S.camera(), S.camera((0.02, 0.04, -0.03), (2.0, -1.2, 1.8)), S.camera((-0.04, -0.02, 0.05), (2.8, -1.8, 1.2)),
           S.camera((0.05, 0.06, 0.01), (2.2, -1.6, 2.0))]


def synthetic_features(n, seed):
    """n features spread over the image with octaves 0..7 and random descriptors (no extraction: usable without a GPU)."""
    rng = np.random.default_rng(seed)
    return dict(kx=rng.uniform(16, 736, n).astype("f4"), ky=rng.uniform(16, 464, n).astype("f4"),
                oct=rng.choice(8, n, p=[.3, .2, .15, .1, .1, .05, .05, .05]).astype("i4"), desc=rng.integers(0, 256, (n, 32), dtype=np.uint8))


def cut(feat, idx):
    return {k: np.ascontiguousarray(np.asarray(feat[k])[idx]) for k in ("kx", "ky", "oct", "desc")}


def make_scene(feats, n_points, n_match, n_hold, seed, spare=7, cams=None):
    """K keyframes (feats[k] = dict(kx, ky, oct, desc)) under cams[k] (default CAMERAS[k]), and n_points map points in a table of n_points + spare
    slots: the first n_match features of every keyframe back-projected through its pose (S.matchable_points), then random distractors
    (S.random_points), shuffled, cut to n_points and stored in permuted slots.  A twentieth of the rows is BAD, another is not LIVE.
    The first n_hold features of every keyframe hold their own point (where it made the cut); two more hold ids outside the table.
    Returns dict(kfs = [dict(kx, ky, oct, desc, Tcw, Ow, mp_id)], rows (over all slots), slots [n_points], capacity)."""
    rng = np.random.default_rng(seed)
    cams = CAMERAS if cams is None else cams
    parts, owner = [], []
    for k, f in enumerate(feats):
        m = min(n_match, len(f["kx"]))
        if m:
            parts.append(S.matchable_points(f["kx"][:m], f["ky"][:m], f["oct"][:m], f["desc"][:m], *cams[k], seed=seed + k))
            owner += [(k, i) for i in range(m)]
    n_rand = max(n_points - len(owner), n_points // 4 + 1)
    parts.append(S.random_points(n_rand, seed + 100))
    owner += [(-1, -1)] * n_rand
    pool = S.concat(*parts)
    pick = rng.permutation(len(owner))[:n_points]
    cap = n_points + spare
    slots = rng.permutation(cap)[:n_points].astype("i4")
    rows = dict(pos=np.zeros((cap, 3), "f4"), normal=np.zeros((cap, 3), "f4"), min_dist=np.zeros(cap, "f4"), max_dist=np.zeros(cap, "f4"),
                desc=np.zeros((cap, 32), np.uint8), flags=np.zeros(cap, np.uint8))
    for c in COLS:
        rows[c][slots] = pool[c][pick]
    kind = rng.random(n_points)
    rows["flags"][slots[kind < 0.05]] |= BAD
    rows["flags"][slots[(kind >= 0.05) & (kind < 0.10)]] &= ~np.uint8(LIVE)
    kfs = []
    for k, f in enumerate(feats):
        ids = np.full(len(f["kx"]), -1, "i4")
        for j, p in enumerate(pick):
            kk, i = owner[p]
            if kk == k and i < n_hold:
                ids[i] = slots[j]
        if len(ids) > n_hold + 2:
            ids[n_hold] = cap; ids[n_hold + 1] = 1 << 30          # ids outside the table: ignored
        kfs.append(dict(cut(f, slice(None)), Tcw=cams[k][0], Ow=cams[k][1], mp_id=ids))
    return dict(kfs=kfs, rows=rows, slots=slots, capacity=cap)


def big_scene():
    """4 keyframes x 1000 synthetic features x 3000 points: 550 matchable points per keyframe, 100 of them held, 800 distractors."""
    return make_scene([synthetic_features(1000, 40 + k) for k in range(4)], 3000, 550, 100, seed=9)


PARAMS = (dict(th=3.0, chi2_check=True, accept_th=50), dict(th=4.0, chi2_check=False, accept_th=50))   # Fuse(pKF, points); Fuse(pKF, Scw, ...)


def _x_with(target):
    """The float x with fx * (x * 1) + cx == target exactly (identity camera, z = 1)."""
    fx, cx = F(INTR[0]), F(INTR[2])
    x = F(F(target - INTR[2]) / fx)
    for _ in range(8):
        if fx * x + cx == F(target):
            return x
        x = np.nextafter(x, F(np.inf) if fx * x + cx < F(target) else F(-np.inf))
    raise AssertionError("no float projects to %r" % target)


def association_row(seed=1, tries=100000):
    """(X, Z) with fx * ((X * invz)) + cx != (fx * X) * invz + cx in float32: Fuse's reading against isInFrustum's."""
    rng = np.random.default_rng(seed)
    fx, cx = F(INTR[0]), F(INTR[2])
    X = rng.uniform(-1, 1, tries).astype("f4"); Z = rng.uniform(2, 6, tries).astype("f4")
    invz = F(1.0) / Z
    i = np.flatnonzero((fx * (X * invz) + cx) != (fx * X * invz + cx))
    assert len(i), "no such row among %d" % tries
    return X[i[0]], Z[i[0]]


def edge_points():
    """Hand-built rows for the identity camera (Tcw = [I | 0], Ow = 0):
    row 0: the camera centre, Pc = 0 (u = NaN: OUTSIDE);  row 1: u == max_x exactly (OUTSIDE);  row 2: u == min_x exactly (kept);
    row 3: dot == 0.5 * dist exactly (kept);  row 4: the association row;  rows 5..68: the level boundaries of
    S.edge_points() (dist = 2, max_dist / dist = float32(1.2)^k nudged by -4..+3 ulps)."""
    e = S.edge_points()
    X, Z = association_row()
    pos = np.array([[0, 0, 0], [_x_with(BOUNDS[1]), 0, 1], [_x_with(BOUNDS[0]), 0, 1], [0, 0, 2], [X, 0, Z]], "f4")
    normal = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0.5], [0, 0, 1]], "f4")
    mx = np.array([4, 4, 4, 4, 8], "f4")
    rng = np.random.default_rng(5)
    n = 5 + 64
    return dict(pos=np.concatenate([pos, e["pos"][2:]]), normal=np.concatenate([normal, e["normal"][2:]]), min_dist=np.full(n, 0.01, "f4"),
                max_dist=np.concatenate([mx, e["max_dist"][2:]]), desc=rng.integers(0, 256, (n, 32), dtype=np.uint8),
                flags=np.full(n, LIVE | HAS_OBS, np.uint8))
