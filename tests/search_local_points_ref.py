"""numpy restatement of ccm_frame_search_local_points (include/ccm_hot.h): Frame::isInFrustum (src/Frame.cpp:139-198) and
MapPoint::PredictScale (src/MapPoint.cpp:854-869) in float32 storage with float64 sums, the query set-up of
ORBmatcher::SearchByProjection (ORBmatcher.cpp:97-107), a sequential replay of Tracking::SearchLocalPoints
(src/Tracking.cpp:860-922), and the scenes the tests use.  Shared by test_map_table_cpu.py, test_search_local_points_gpu.py and
tools/bench_search_local_points.py; nothing here touches the GPU."""
import numpy as np

F = np.float32
LIVE, BAD, HAS_OBS = 1, 2, 4
INTR = (458.0, 457.0, 367.0, 248.0)
BOUNDS = (0.0, 752.0, 0.0, 480.0)                 # mnMinX, mnMaxX, mnMinY, mnMaxY
N_LEVELS = 8
SCALE = np.cumprod(np.concatenate([[F(1.0)], np.full(N_LEVELS - 1, F(1.2))]).astype("f4")).astype("f4")   # mvScaleFactors
LOG_SF = F(np.log(np.float64(F(1.2))))            # mfLogScaleFactor = log(mfScaleFactor)
GATES = ("in view", "PcZ < 0", "u outside", "v outside", "distance", "viewing angle")


def camera(rotvec=(0.03, -0.05, 0.02), t=(2.5, -1.5, 1.5)):
    """Tcw [3][4] float32 of a slightly rotated camera and Ow = -Rcw^T tcw (sums in double, stored as float).  The camera stands
    2 to 3 units off the cloud of reference centres, so that the distance and the viewing-angle tests reject points too."""
    w = np.asarray(rotvec, "f8"); th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / (th if th else 1.0)
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T = np.concatenate([R, np.asarray(t, "f8")[:, None]], 1).astype("f4")
    Ow = (-(T[:, :3].astype("f8").T) @ T[:, 3].astype("f8")).astype("f4")
    return T, Ow


def frustum(pos, normal, min_dist, max_dist, Tcw, Ow, intr=INTR, bounds=BOUNDS, cos_limit=0.5, log_sf=LOG_SF, n_levels=N_LEVELS):
    """isInFrustum + PredictScale for every row.  Returns dict(gate [M] int: 0 = in view, 1..5 = the rejecting test in the
    reference's order, u, v, dist, view_cos, level, ambiguous) -- values past the rejecting test are meaningless."""
    P = np.ascontiguousarray(pos, "f4").reshape(-1, 3); Pn = np.ascontiguousarray(normal, "f4").reshape(-1, 3)
    mn = np.ascontiguousarray(min_dist, "f4"); mx = np.ascontiguousarray(max_dist, "f4")
    T = np.asarray(Tcw, "f4").reshape(3, 4); Ow = np.asarray(Ow, "f4")
    fx, fy, cx, cy = [F(v) for v in intr]; x0, x1, y0, y1 = [F(v) for v in bounds]
    Pd = P.astype("f8"); Td = T.astype("f8")
    with np.errstate(all="ignore"):
        Pc = np.stack([((Td[r, 0] * Pd[:, 0] + Td[r, 1] * Pd[:, 1]) + Td[r, 2] * Pd[:, 2]) + Td[r, 3] for r in range(3)], 1).astype("f4")
        invz = F(1.0) / Pc[:, 2]
        u = fx * Pc[:, 0] * invz + cx
        v = fy * Pc[:, 1] * invz + cy
        PO = P - Ow[None, :]
        POd = PO.astype("f8")
        dist = np.sqrt((POd[:, 0] * POd[:, 0] + POd[:, 1] * POd[:, 1]) + POd[:, 2] * POd[:, 2]).astype("f4")
        Nd = Pn.astype("f8")
        vc = (((POd[:, 0] * Nd[:, 0] + POd[:, 1] * Nd[:, 1]) + POd[:, 2] * Nd[:, 2]) / dist.astype("f8")).astype("f4")
        ratio = mx / dist
        lg = np.log(ratio.astype("f8")).astype("f4")

        def lvl(l):
            c = np.ceil(l / F(log_sf))
            return np.where(~(c >= 0), 0, np.where(c >= n_levels, n_levels - 1, c)).astype("i4")
        level = lvl(lg)
        amb = (lvl(np.nextafter(lg, F(np.inf))) != level) | (lvl(np.nextafter(lg, F(-np.inf))) != level)
        gate = np.zeros(len(P), "i4")
        for k, rej in ((5, vc < F(cos_limit)), (4, (dist < F(0.8) * mn) | (dist > F(1.2) * mx)), (3, (v < y0) | (v > y1)),
                       (2, (u < x0) | (u > x1)), (1, Pc[:, 2] < 0)):
            gate[rej] = k                         # the earliest test wins: assigned last
    return dict(gate=gate, u=u, v=v, dist=dist, view_cos=vc, level=level, ambiguous=amb & (gate == 0))


def queries(view_cos, level, scale=SCALE, th=1.0):
    """window_queries_projection(): radius (RadiusByViewingCos, * th unless th == 1, * scale[level]) and the level window."""
    r = np.where(np.asarray(view_cos, "f4").astype("f8") > 0.998, F(2.5), F(4.0)).astype("f4")
    if th != 1.0:
        r = r * F(th)
    lv = np.asarray(level, "i4")
    return (r * np.asarray(scale, "f4")[lv]).astype("f4"), lv - 1, lv.copy()


def replay(frame_ids, rows, order, Tcw, Ow, **kw):
    """The two loops of Tracking::SearchLocalPoints, sequentially.  rows = dict(pos, normal, min_dist, max_dist, desc, flags) over all
    slots; order = the visiting order (None: ascending slot over the LIVE slots).  Returns dict(ids, occupied, in_view_slot, proj_x,
    proj_y, level, view_cos, ambiguous, has_obs, desc) -- the last seven per entry in view, in visiting order."""
    flags = np.asarray(rows["flags"], np.uint8)
    ids = np.asarray(frame_ids, "i4").copy()
    occupied = np.zeros(len(ids), np.uint8)
    seen = np.zeros(len(flags), bool)
    for i, s in enumerate(ids):                                   # :863-879
        if s < 0:
            continue
        assert flags[s] & LIVE
        if flags[s] & BAD:
            ids[i] = -1
        else:
            seen[s] = True
            occupied[i] = 1 if flags[s] & HAS_OBS else 0
    if order is None:
        order = np.flatnonzero(flags & LIVE)
    order = np.asarray(order, "i4")
    fr = frustum(rows["pos"], rows["normal"], rows["min_dist"], rows["max_dist"], Tcw, Ow, **kw)
    fl = flags[order]
    keep = ((fl & LIVE) != 0) & ((fl & BAD) == 0) & ~seen[order] & (fr["gate"][order] == 0)      # :888-908
    iv = order[keep]
    return dict(ids=ids, occupied=occupied, in_view_slot=iv, proj_x=fr["u"][iv], proj_y=fr["v"][iv], level=fr["level"][iv],
                view_cos=fr["view_cos"][iv], ambiguous=fr["ambiguous"][iv], has_obs=((flags[iv] & HAS_OBS) != 0),
                desc=np.asarray(rows["desc"], np.uint8)[iv], gate=fr["gate"])


# ------------------------------------------------------------------------------------------------------------------ scenes
def random_points(M, seed):
    """M random points in a box around the camera (x in [-8, 8], y in [-5, 5], z in [-3, 14]): reference centres N(0, 1), normals =
    the unit ray from the reference centre with sigma = 0.15 noise, max_dist = dist_ref * 1.2^level with level uniform in 0..7,
    min_dist = max_dist / 1.2^7."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-8, 8, M), rng.uniform(-5, 5, M), rng.uniform(-3, 14, M)], 1)
    ref = rng.normal(0, 1, (M, 3))
    ray = pos - ref
    dref = np.linalg.norm(ray, axis=1)
    normal = ray / dref[:, None] + rng.normal(0, 0.15, (M, 3))
    mx = dref * 1.2 ** rng.integers(0, 8, M)
    return dict(pos=pos.astype("f4"), normal=normal.astype("f4"), min_dist=(mx / 1.2 ** 7).astype("f4"), max_dist=mx.astype("f4"),
                desc=rng.integers(0, 256, (M, 32), dtype=np.uint8),
                flags=np.where(rng.random(M) < 0.9, LIVE | HAS_OBS, LIVE).astype(np.uint8))


def matchable_points(kx, ky, octave, desc, Tcw, Ow, seed, intr=INTR):
    """One map point per feature of an extracted frame: the feature back-projected through the inverse pose to a random depth
    (computed in double, stored as float), its descriptor with 5 % of the bits flipped, seen from the camera centre, and a distance
    range that predicts the feature's own octave."""
    rng = np.random.default_rng(seed)
    n = len(kx)
    fx, fy, cx, cy = intr
    z = rng.uniform(2, 10, n)
    Pc = np.stack([(np.asarray(kx, "f8") - cx) / fx * z, (np.asarray(ky, "f8") - cy) / fy * z, z], 1)
    T = np.asarray(Tcw, "f8").reshape(3, 4)
    Pw = (Pc - T[:, 3][None, :]) @ T[:, :3]                       # R^T (Pc - t)
    ray = Pw - np.asarray(Ow, "f8")[None, :]
    d = np.linalg.norm(ray, axis=1)
    normal = ray / d[:, None] + rng.normal(0, 0.02, (n, 3))
    mx = d * 1.2 ** (np.asarray(octave, "f8") - 0.5)              # ceil(octave - 0.5) = octave; octave 0 clamps to 0
    flips = np.packbits(rng.random((n, 256)) < 0.05, axis=1, bitorder="little")
    return dict(pos=Pw.astype("f4"), normal=normal.astype("f4"), min_dist=(mx / 1.2 ** 7).astype("f4"), max_dist=mx.astype("f4"),
                desc=np.asarray(desc, np.uint8) ^ flips, flags=np.where(rng.random(n) < 0.95, LIVE | HAS_OBS, LIVE).astype(np.uint8))


def edge_points():
    """Hand-built rows for the identity camera (Tcw = [I | 0], Ow = 0), with what must happen to each:
    row 0: on the camera plane with PcX != 0 (invz = inf, u = inf: rejected by the u test, not the depth test);
    row 1: u == max_x exactly (kept: the test is u > max_x);  rows 2..65: dist = 2 and max_dist / dist = float32(1.2)^k nudged by
    -4..+3 ulps, k = 0..7 (the level boundaries of PredictScale)."""
    fx, fy, cx, cy = [F(v) for v in INTR]
    x = F(F(BOUNDS[1] - INTR[2]) / fx)
    for _ in range(8):                                            # the float whose projection is exactly max_x
        if fx * x * F(1.0) + cx == F(BOUNDS[1]):
            break
        x = np.nextafter(x, F(np.inf) if fx * x + cx < F(BOUNDS[1]) else F(-np.inf))
    assert fx * x * F(1.0) + cx == F(BOUNDS[1])
    pos = [[1.0, 0.5, 0.0], [x, 0.0, 1.0]]
    mx = [4.0, 2.0]
    for k in range(8):
        r = F(1.0)
        for _ in range(k):
            r = F(r * F(1.2))
        for nudge in range(-4, 4):
            rr = r
            for _ in range(abs(nudge)):
                rr = np.nextafter(rr, F(np.inf) if nudge > 0 else F(-np.inf))
            pos.append([0.0, 0.0, 2.0]); mx.append(F(2.0) * rr)
    pos = np.array(pos, "f4"); mx = np.array(mx, "f4")
    n = len(pos)
    rng = np.random.default_rng(5)
    normal = pos / np.maximum(np.linalg.norm(pos, axis=1), 1e-9)[:, None]
    return dict(pos=pos, normal=normal.astype("f4"), min_dist=np.full(n, 0.01, "f4"), max_dist=mx,
                desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), flags=np.full(n, LIVE | HAS_OBS, np.uint8))


IDENTITY = (np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype("f4"), np.zeros(3, "f4"))


def concat(*rows):
    return {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
