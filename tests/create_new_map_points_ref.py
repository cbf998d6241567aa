"""Float64 numpy restatement of LocalMapping::CreateNewMapPoints (src/Mapping.cpp:312-468) and the scenes of its tests.

Test infrastructure: nothing here is imported by the library.

  pairs_ref        :363-448 for the matched pairs of one neighbour, in float64, with the ambiguity flags
  emulate_pairs32  the same in float32 storage in the operation order of csrc/map_math.h (tools/create_new_map_points_study.py)
  gates32          :399-448 from a given float32 point, bit for bit what map_gates computes
  resolve          "a feature belongs to the first neighbour whose pair passes every gate"
  create_new_map_points   the reference's sequential loop around a SearchForTriangulation function and a pair function
  make_scene       the seeded scene of the GPU test, make_small the small cases

A pair is AMBIGUOUS when a gate the float64 evaluation reaches lies within a band of its threshold: 1e-5 absolute for the two cosine
tests and for depth / |X - O| against 0, 1e-3 relative for the two reprojection tests, 1e-4 relative for the two scale tests.

The scene follows the recipe this feature was specified with (camera 752 x 480, f = 458, 8 levels of 1.2; points in x [-6, 6], y [-3, 3],
z [4, 14]; 20 neighbours with rotations of sigma 0.03 rad and baselines 0.02 m, 0.1 m and 18 from [0.15, 1.2] m; octave from the
depth per view; pixel noise 0.5 * 1.2^octave; 6 % second octaves off by +-4, 10 % slid along the epipolar line by up to +-60 px,
8 % displaced across it by 3-9 sigma; 256-bit descriptors with ~6 % flips per view; nodes in [0, 60) kept across views for ~90 %;
40 % / 30 % map-point flags) with three differences, each forced by what the GPU test has to cover:
  * 4200 points instead of 1200.  With 40 % of the current features holding a map point, 1200 points leave about 500 features that
    can win at all, and the test asks for 1000 OK rows.
  * A pair displaced across the epipolar line by 3 sigma or more never passes CheckDistEpipolarLine (1.96 sigma), so through the
    matcher that class ends as NO_MATCH.  The pairs fed directly to the math check (CPU test) reach REPROJ_1 / REPROJ_2 with it; for
    the GPU test 20 % of the second observations of near points (octave 0 or 1) are given octave 7 and displaced by 1.6-1.9 sigma of
    that octave: inside the epipolar gate of the coarse octave (1.96 sigma_2), outside the reprojection gate of the fine one (the
    triangulation leaves about half of the offset in each view, and 0.8 * 3.58 px > 2.45 * 1.2 px).  REPROJ_2 cannot be reached
    through the matcher at all: its gate is wider than the epipolar gate that the same observation has already passed.
  * Neighbour 20 stands 8 m in front of the current keyframe and looks the same way: points nearer than that project through its
    pinhole with negative depth, which is what reaches BEHIND_2.
"""
import numpy as np

SEED = 20261017
W, H, FX, FY, CX, CY = 752, 480, 458.0, 458.0, 376.0, 240.0
N_LEVELS, SCALE = 8, 1.2
SCALE_FACTORS = (SCALE ** np.arange(N_LEVELS)).astype("f4")
LEVEL_SIGMA2 = (SCALE_FACTORS * SCALE_FACTORS).astype("f4")
STATUS = ("SKIPPED_KF", "HAS_MP", "NO_MATCH", "LOW_PARALLAX", "W_ZERO", "NONFINITE", "BEHIND_1", "BEHIND_2", "REPROJ_1", "REPROJ_2",
          "ZERO_DIST", "SCALE", "OK", "SUPERSEDED")
S = {name: i for i, name in enumerate(STATUS)}
# the GPU test's small cases: (n1, neighbours, options of make_small); n_kf = 1, 2, 3 and n1 = 1, 63, 64, 65, a neighbour without
# features, a neighbour that shares no node with the current keyframe, every current feature already holding a map point
SMALL_CASES = ((1, (2,), {}), (63, (2, 7), {}), (64, (3, 8, 9), {}), (65, (4,), {}), (64, (5, 6, 9), dict(empty=1)),
               (65, (4, 6), dict(foreign=0)), (64, (3, 10), dict(all_flagged=True)))
RANGE_NODE, RANGE_SIZES = 60, {2: 63, 3: 64, 4: 65, 5: 130}          # node 60 holds this many candidate features in these neighbours


# ------------------------------------------------------------------ geometry helpers
def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def f12_64(T1, T2, K1, K2):
    """ComputeF12 (:549-566) in float64 from [R|t] 3x4 and (fx, fy, cx, cy)."""
    R12 = T1[:, :3] @ T2[:, :3].T
    t12 = -R12 @ T2[:, 3] + T1[:, 3]
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Km = lambda K: np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    return np.linalg.inv(Km(K1).T) @ tx @ R12 @ np.linalg.inv(Km(K2))


def baseline_too_short(Ow1, Ow2, median_depth):
    """:319-328 in float64"""
    return np.linalg.norm(np.asarray(Ow2, "f8") - np.asarray(Ow1, "f8")) / float(median_depth) < 0.01


# ------------------------------------------------------------------ :363-448 in float64
def pairs_ref(kf1, kf2, i1, i2):
    """-> dict(status [m], X [m][3], ambiguous [m] bool, z1 [m]) for the pairs (i1[j], i2[j]) of keyframes kf1, kf2 (dicts of make_scene)."""
    i1 = np.asarray(i1, "i8"); i2 = np.asarray(i2, "i8"); m = len(i1)
    out = dict(status=np.full(m, S["OK"], "i4"), X=np.zeros((m, 3)), ambiguous=np.zeros(m, bool), z1=np.ones(m))
    if m == 0:
        return out
    T1, T2 = kf1["Tcw"].astype("f8"), kf2["Tcw"].astype("f8")
    K1, K2 = kf1["K"].astype("f8"), kf2["K"].astype("f8")
    O1, O2 = kf1["Ow"].astype("f8"), kf2["Ow"].astype("f8")
    x1, y1, x2, y2 = (a.astype("f8") for a in (kf1["kp_x"][i1], kf1["kp_y"][i1], kf2["kp_x"][i2], kf2["kp_y"][i2]))
    o1, o2 = kf1["kp_octave"][i1], kf2["kp_octave"][i2]
    sig1, sig2 = kf1["level_sigma2"].astype("f8")[o1], kf2["level_sigma2"].astype("f8")[o2]
    sf1, sf2 = kf1["scale_factors"].astype("f8")[o1], kf2["scale_factors"].astype("f8")[o2]
    ratio_factor = 1.5 * float(kf1["scale_factors"][1])
    xn1 = np.stack([(x1 - K1[2]) / K1[0], (y1 - K1[3]) / K1[1], np.ones(m)], 1)
    xn2 = np.stack([(x2 - K2[2]) / K2[0], (y2 - K2[3]) / K2[1], np.ones(m)], 1)
    ray1, ray2 = xn1 @ T1[:, :3], xn2 @ T2[:, :3]                     # Rwc * xn = (xn^T Rcw)^T
    cos = (ray1 * ray2).sum(1) / (np.linalg.norm(ray1, axis=1) * np.linalg.norm(ray2, axis=1))
    status, amb = out["status"], out["ambiguous"]
    live = np.ones(m, bool)

    def gate(fail, code, near):
        nonlocal live
        amb[live & near] = True
        status[live & fail] = code
        live = live & ~fail

    with np.errstate(all="ignore"):
        gate(~((cos > 0) & (cos < 0.9998)), S["LOW_PARALLAX"], (np.abs(cos) < 1e-5) | (np.abs(cos - 0.9998) < 1e-5))
        A = np.stack([xn1[:, :1] * T1[2] - T1[0], xn1[:, 1:2] * T1[2] - T1[1], xn2[:, :1] * T2[2] - T2[0], xn2[:, 1:2] * T2[2] - T2[1]], 1)
        v = np.linalg.svd(A)[2][:, 3, :]
        gate(v[:, 3] == 0, S["W_ZERO"], np.zeros(m, bool))
        X = v[:, :3] / v[:, 3:4]
        gate(~np.isfinite(X).all(1), S["NONFINITE"], np.zeros(m, bool))
        X = np.where(np.isfinite(X), X, 0.0)
        out["X"][:] = np.where((status >= S["NONFINITE"])[:, None], X, 0.0)
        d1, d2 = np.linalg.norm(X - O1, axis=1), np.linalg.norm(X - O2, axis=1)
        z1 = X @ T1[2, :3] + T1[2, 3]
        out["z1"][:] = z1
        gate(z1 <= 0, S["BEHIND_1"], np.abs(z1) < 1e-5 * d1)
        z2 = X @ T2[2, :3] + T2[2, 3]
        gate(z2 <= 0, S["BEHIND_2"], np.abs(z2) < 1e-5 * d2)
        e1 = (K1[0] * (X @ T1[0, :3] + T1[0, 3]) / z1 + K1[2] - x1) ** 2 + (K1[1] * (X @ T1[1, :3] + T1[1, 3]) / z1 + K1[3] - y1) ** 2
        gate(e1 > 5.991 * sig1, S["REPROJ_1"], np.abs(e1 / (5.991 * sig1) - 1) < 1e-3)
        e2 = (K2[0] * (X @ T2[0, :3] + T2[0, 3]) / z2 + K2[2] - x2) ** 2 + (K2[1] * (X @ T2[1, :3] + T2[1, 3]) / z2 + K2[3] - y2) ** 2
        gate(e2 > 5.991 * sig2, S["REPROJ_2"], np.abs(e2 / (5.991 * sig2) - 1) < 1e-3)
        gate((d1 == 0) | (d2 == 0), S["ZERO_DIST"], np.zeros(m, bool))
        rd, ro = d2 / d1, sf1 / sf2
        gate((rd * ratio_factor < ro) | (rd > ro * ratio_factor), S["SCALE"],
             (np.abs(rd * ratio_factor / ro - 1) < 1e-4) | (np.abs(rd / (ro * ratio_factor) - 1) < 1e-4))
    return out


# ------------------------------------------------------------------ float32 storage, the operation order of csrc/map_math.h
F4, F8 = np.float32, np.float64


def _row32(T, r, X):
    d = T[r, 0].astype(F8) * X[:, 0].astype(F8) + T[r, 1].astype(F8) * X[:, 1].astype(F8) + T[r, 2].astype(F8) * X[:, 2].astype(F8)
    return (d + T[r, 3].astype(F8)).astype(F4)


def _norm32(v):
    v = v.astype(F8)
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def gates32(kf1, kf2, i1, i2, X):
    """map_gates of csrc/map_math.h in numpy: the status (BEHIND_1 .. OK) of each pair from the float32 point X [m][3]."""
    i1 = np.asarray(i1, "i8"); i2 = np.asarray(i2, "i8"); m = len(i1)
    X = np.ascontiguousarray(X, F4)
    T1, T2, K1, K2, O1, O2 = kf1["Tcw"], kf2["Tcw"], kf1["K"], kf2["K"], kf1["Ow"], kf2["Ow"]
    status = np.full(m, S["OK"], "i4"); live = np.ones(m, bool)

    def gate(fail, code):
        nonlocal live
        status[live & fail] = code
        live = live & ~fail

    with np.errstate(all="ignore"):
        z1 = _row32(T1, 2, X); gate(z1 <= 0, S["BEHIND_1"])
        z2 = _row32(T2, 2, X); gate(z2 <= 0, S["BEHIND_2"])
        for T, K, z, kf, idx, code in ((T1, K1, z1, kf1, i1, S["REPROJ_1"]), (T2, K2, z2, kf2, i2, S["REPROJ_2"])):
            x, y = _row32(T, 0, X), _row32(T, 1, X)
            invz = (1.0 / z.astype(F8)).astype(F4)
            u = K[0] * x * invz + K[2]; v = K[1] * y * invz + K[3]
            ex = u - kf["kp_x"][idx]; ey = v - kf["kp_y"][idx]
            sig = kf["level_sigma2"][kf["kp_octave"][idx]]
            gate((ex * ex + ey * ey).astype(F8) > 5.991 * sig.astype(F8), code)
        d1 = _norm32(X - O1).astype(F4); d2 = _norm32(X - O2).astype(F4)
        gate((d1 == 0) | (d2 == 0), S["ZERO_DIST"])
        rd = d2 / d1
        ro = kf1["scale_factors"][kf1["kp_octave"][i1]] / kf2["scale_factors"][kf2["kp_octave"][i2]]
        rf = F4(1.5) * kf1["scale_factors"][1]
        gate((rd * rf < ro) | (rd > ro * rf), S["SCALE"])
    return status


def emulate_pairs32(kf1, kf2, i1, i2):
    """map_pair of csrc/map_math.h in numpy (LAPACK's eigh instead of the Jacobi sweeps: both work in double on the same A^T A)."""
    i1 = np.asarray(i1, "i8"); i2 = np.asarray(i2, "i8"); m = len(i1)
    status = np.full(m, S["OK"], "i4"); X = np.zeros((m, 3), F4)
    if m == 0:
        return dict(status=status, X=X)
    T1, T2, K1, K2 = kf1["Tcw"], kf2["Tcw"], kf1["K"], kf2["K"]
    one = np.ones(m, F4)
    xn1 = np.stack([(kf1["kp_x"][i1] - K1[2]) * (F4(1) / K1[0]), (kf1["kp_y"][i1] - K1[3]) * (F4(1) / K1[1]), one], 1)
    xn2 = np.stack([(kf2["kp_x"][i2] - K2[2]) * (F4(1) / K2[0]), (kf2["kp_y"][i2] - K2[3]) * (F4(1) / K2[1]), one], 1)
    ray = lambda T, xn: np.stack([T[0, r].astype(F8) * xn[:, 0].astype(F8) + T[1, r].astype(F8) * xn[:, 1].astype(F8)
                                  + T[2, r].astype(F8) * xn[:, 2].astype(F8) for r in range(3)], 1).astype(F4)
    r1, r2 = ray(T1, xn1), ray(T2, xn2)
    a, b = r1.astype(F8), r2.astype(F8)
    with np.errstate(all="ignore"):
        cos = ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]) / (_norm32(r1) * _norm32(r2))).astype(F4)
        low = ~((cos < cos + F4(1)) & (cos > 0) & (cos.astype(F8) < 0.9998))
        A = np.stack([xn1[:, :1] * T1[2] - T1[0], xn1[:, 1:2] * T1[2] - T1[1], xn2[:, :1] * T2[2] - T2[0], xn2[:, 1:2] * T2[2] - T2[1]], 1)
        assert A.dtype == F4
        A8 = A.astype(F8)
        v = np.linalg.eigh(np.einsum("mri,mrj->mij", A8, A8))[1][:, :, 0].astype(F4)
        wz = v[:, 3] == 0
        P = v[:, :3] / v[:, 3:4]
        nf = ~np.isfinite(P).all(1)
        g = gates32(kf1, kf2, i1, i2, np.where(np.isfinite(P), P, F4(0)))
    status[:] = np.where(low, S["LOW_PARALLAX"], np.where(wz, S["W_ZERO"], np.where(nf, S["NONFINITE"], g)))
    X[:] = np.where((status >= S["NONFINITE"])[:, None], P, F4(0))
    return dict(status=status, X=X)


# ------------------------------------------------------------------ the ordered part
def resolve(gate_ok):
    """gate_ok [n_kf][n1] bool (the pair of (k, i1) passes every gate) -> winner [n1]: the first such k, or -1."""
    gate_ok = np.asarray(gate_ok, bool)
    if gate_ok.shape[0] == 0:
        return np.full(gate_ok.shape[1], -1, "i4")
    return np.where(gate_ok.any(0), gate_ok.argmax(0), -1).astype("i4")


def create_new_map_points(scene, search, pair_status):
    """The loop of :312-468.  search(k, has_mp1) -> match12 [n1] (SearchForTriangulation of the current keyframe, with the map-point
    flags as they stand, against neighbour k); pair_status(k, i1, i2) -> (status [m], X [m][3]).  -> rows (kf, idx1, idx2, x3d) in
    creation order and first [n_kf + 1]."""
    cur = scene["current"]
    has_mp1 = cur["has_mp"].copy()
    rows, first = [], [0]
    for k, kf in enumerate(scene["neighbours"]):
        if not baseline_too_short(cur["Ow"], kf["Ow"], scene["median_depth"][k]):
            m12 = np.asarray(search(k, has_mp1))
            i1 = np.flatnonzero(m12 >= 0); i2 = m12[i1]                   # vMatchedIndices: idx1 ascending (:843-849)
            st, X = pair_status(k, i1, i2)
            for j in np.flatnonzero(np.asarray(st) == S["OK"]):
                rows.append((k, int(i1[j]), int(i2[j]), np.asarray(X[j])))
                has_mp1[i1[j]] = 1                                        # AddMapPoint (:456)
        first.append(len(rows))
    return rows, np.array(first, "i4")


# ------------------------------------------------------------------ scenes
def _project(T, X):
    Xc = X @ T[:, :3].T + T[:, 3]
    return FX * Xc[:, 0] / Xc[:, 2] + CX, FY * Xc[:, 1] / Xc[:, 2] + CY, Xc[:, 2]


def _octave(depth):
    return np.clip(np.round(np.log(np.abs(depth) / 4.0) / np.log(SCALE)), 0, N_LEVELS - 1).astype("i4")


def _keyframe(T, cols):
    T = np.asarray(T, "f8")
    kf = dict(K=np.array([FX, FY, CX, CY], "f4"), Tcw=T.astype("f4"), Ow=(-T[:, :3].T @ T[:, 3]).astype("f4"),
              scale_factors=SCALE_FACTORS, level_sigma2=LEVEL_SIGMA2)
    kf.update(kp_x=cols["x"].astype("f4"), kp_y=cols["y"].astype("f4"), kp_octave=cols["oct"].astype("i4"), desc=cols["desc"].astype("u1"),
              node=cols["node"].astype("i4"), has_mp=cols["has_mp"].astype("u1"), point=cols["point"].astype("i4"))
    return kf


def _flip(rng, desc, share):
    bits = np.unpackbits(desc, axis=1)
    return np.packbits(bits ^ (rng.random(bits.shape) < share).astype("u1"), axis=1)


def _view(rng, T, X, pdesc, pnode, flag_share, behind=False):
    """The features of one keyframe: the points that project inside the image (through the pinhole too when `behind`)."""
    u, v, z = _project(T, X)
    vis = (u > 5) & (u < W - 5) & (v > 5) & (v < H - 5) & ((z > 0.5) | (behind & (z < -0.5)))
    idx = np.flatnonzero(vis)
    idx = idx[rng.permutation(len(idx))]                                   # feature order is not point order
    octv = _octave(z[idx])
    sig = SCALE ** octv
    node = pnode[idx].copy()
    redraw = (rng.random(len(idx)) < 0.10) & (node != RANGE_NODE)
    node[redraw] = rng.integers(0, 60, int(redraw.sum()))
    node[(rng.random(len(idx)) < 0.03) & (node != RANGE_NODE)] = -1
    return dict(x=u[idx] + rng.normal(0, 0.5, len(idx)) * sig, y=v[idx] + rng.normal(0, 0.5, len(idx)) * sig, oct=octv,
                desc=_flip(rng, pdesc[idx], 0.06), node=node, has_mp=(rng.random(len(idx)) < flag_share), point=idx)


def _append(cols, extra):
    return {k: np.concatenate([cols[k], extra[k]]) for k in cols}


def _pose(R, center):
    return np.concatenate([R, (-R @ center)[:, None]], 1)


def make_scene(seed=SEED, n_points=4200, n_kf=21):
    """-> dict(current, neighbours [n_kf], median_depth [n_kf], F12 [n_kf][3][3] float32, X [n_points][3]).  A keyframe is a dict of
    the arrays of ccm_map_keyframe plus point [n] (the 3-D point behind a feature, -1 for clutter) and copy_of [n] (the feature this
    one duplicates exactly, -1)."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-6, 6, n_points), rng.uniform(-3, 3, n_points), rng.uniform(4, 14, n_points)], 1)
    pdesc = rng.integers(0, 256, (n_points, 32)).astype("u1")
    pnode = rng.integers(0, 60, n_points)
    pnode[:12] = RANGE_NODE                                                # a dozen points of the node whose ranges are sized below
    T1 = _pose(rodrigues(rng.normal(0, 0.005, 3)), rng.normal(0, 0.01, 3))
    c = _view(rng, T1, X, pdesc, pnode, 0.40)
    nc = len(c["x"])
    dup = rng.choice(nc, 40, replace=False)                                # exact duplicates in the current keyframe: both choose one idx2
    c = _append(c, {k: c[k][dup] for k in c})
    c["has_mp"][nc:] = False; c["has_mp"][dup] = False
    cur = _keyframe(T1, c)
    cur["copy_of"] = np.concatenate([np.full(nc, -1), dup]).astype("i4")
    O1 = cur["Ow"].astype("f8")
    K = cur["K"].astype("f8")
    baselines = [0.02, 0.1] + list(rng.uniform(0.15, 1.2, 18))
    neighbours, median, F12 = [], [], []
    for k in range(n_kf):
        if k < 20:
            d = rng.normal(0, 1, 3); d[2] *= 0.3; d /= np.linalg.norm(d)
            T2 = _pose(rodrigues(rng.normal(0, 0.03, 3)), O1 + baselines[k] * d)
        else:
            T2 = _pose(np.eye(3), O1 + np.array([0.3, 0.1, 8.0]))          # 8 m ahead, the same heading
        n = _view(rng, T2, X, pdesc, pnode, 0.30, behind=k >= 20)
        m = len(n["x"])
        F = f12_64(T1, T2, K, K)
        # ---- stressed pairs: changes to this neighbour's observation of a point
        u = rng.random(m)
        off = u < 0.06
        n["oct"][off] = np.clip(n["oct"][off] + rng.choice([-4, 4], int(off.sum())), 0, N_LEVELS - 1)
        # the epipolar line in this image of the point's (noise-free) projection into the current keyframe
        u1, v1, _ = _project(T1, X[n["point"]])
        line = np.stack([u1, v1, np.ones(m)], 1) @ F
        nrm = np.hypot(line[:, 0], line[:, 1]) + 1e-30
        along = np.stack([-line[:, 1], line[:, 0]], 1) / nrm[:, None]; across = np.stack([line[:, 0], line[:, 1]], 1) / nrm[:, None]
        slide = (u >= 0.06) & (u < 0.16)
        s = rng.uniform(-60, 60, m) * slide
        n["x"] += s * along[:, 0]; n["y"] += s * along[:, 1]
        wide = (u >= 0.16) & (u < 0.24)
        a = rng.uniform(3, 9, m) * rng.choice([-1, 1], m) * SCALE ** n["oct"] * wide
        inside = (u >= 0.24) & (u < 0.44) & (n["oct"] <= 1)                # a near point seen at the coarsest octave: inside its epipolar gate
        n["oct"][inside] = N_LEVELS - 1
        a += rng.uniform(1.6, 1.9, m) * rng.choice([-1, 1], m) * SCALE ** n["oct"] * inside
        n["x"] += a * across[:, 0]; n["y"] += a * across[:, 1]
        # ---- exact duplicates (equal distances: the later index wins) and the sized ranges of RANGE_NODE
        free = np.flatnonzero(~n["has_mp"] & (n["node"] >= 0))
        dup = rng.choice(free, min(25, len(free)), replace=False)
        n = _append(n, {key: n[key][dup] for key in n})
        copy_of = np.concatenate([np.full(m, -1), dup])
        if k in RANGE_SIZES:
            have = int((~n["has_mp"] & (n["node"] == RANGE_NODE)).sum())
            extra = RANGE_SIZES[k] - have
            assert extra >= 0, (k, have)
            cl = dict(x=rng.uniform(10, W - 10, extra), y=rng.uniform(10, H - 10, extra), oct=rng.integers(0, N_LEVELS, extra).astype("i4"),
                      desc=rng.integers(0, 256, (extra, 32)).astype("u1"), node=np.full(extra, RANGE_NODE), has_mp=np.zeros(extra, bool),
                      point=np.full(extra, -1))
            src = np.flatnonzero(n["node"] == RANGE_NODE)
            if len(src):                                                   # a third of the clutter resembles a real feature: candidates past lane 64
                pick = src[rng.integers(0, len(src), extra // 3)]
                cl["desc"][:extra // 3] = _flip(rng, n["desc"][pick], 0.02)
                cl["x"][:extra // 3] = n["x"][pick]; cl["y"][:extra // 3] = n["y"][pick]; cl["oct"][:extra // 3] = n["oct"][pick]
            n = _append(n, cl)
            copy_of = np.concatenate([copy_of, np.full(extra, -1)])
        kf = _keyframe(T2, n)
        kf["copy_of"] = copy_of.astype("i4")
        neighbours.append(kf)
        zc = _project(T2, X)[2]
        median.append(np.float32(np.median(np.abs(zc))))
        F12.append(f12_64(cur["Tcw"].astype("f8"), kf["Tcw"].astype("f8"), K, K).astype("f4"))
    return dict(current=cur, neighbours=neighbours, median_depth=np.array(median, "f4"), F12=np.array(F12, "f4"), X=X)


def epipole32(cur, kf):
    """ORBmatcher.cpp:708-714 in float32"""
    C2 = (kf["Tcw"][:, :3].astype("f8") @ cur["Ow"].astype("f8")).astype("f4") + kf["Tcw"][:, 3]
    invz = np.float32(1.0) / C2[2]
    return np.array([kf["K"][0] * C2[0] * invz + kf["K"][2], kf["K"][1] * C2[1] * invz + kf["K"][3]], "f4")


def subset(kf, idx):
    """The keyframe with the features idx only."""
    out = dict(kf)
    for key in ("kp_x", "kp_y", "kp_octave", "desc", "node", "has_mp", "point", "copy_of"):
        out[key] = kf[key][idx].copy()
    return out


def make_small(scene, n1, ks, all_flagged=False, empty=None, foreign=None):
    """A small case cut from the scene: the first n1 free features of the current keyframe that have a node (all of them flagged when
    all_flagged), the neighbours ks; neighbour `empty` loses its features, neighbour `foreign` gets nodes the current keyframe has
    not."""
    cur = scene["current"]
    pick = np.flatnonzero((cur["has_mp"] == 0) & (cur["node"] >= 0))[:n1]
    c = subset(cur, pick)
    if all_flagged:
        c["has_mp"][:] = 1
    nb = []
    for j, k in enumerate(ks):
        kf = subset(scene["neighbours"][k], np.arange(len(scene["neighbours"][k]["kp_x"])))
        if empty == j:
            kf = subset(kf, np.arange(0))
        if foreign == j:
            kf["node"] = np.where(kf["node"] >= 0, kf["node"] + 1000, -1).astype("i4")
        nb.append(kf)
    ks = list(ks)
    return dict(current=c, neighbours=nb, median_depth=scene["median_depth"][ks].copy(), F12=scene["F12"][ks].copy(), X=scene["X"])


# ------------------------------------------------------------------ pairs for the host check of csrc/map_math.h
def true_pairs(scene, k):
    """The pairs (i1, i2) of the current keyframe and neighbour k that observe one 3-D point (no matcher), first occurrence each."""
    cur, kf = scene["current"], scene["neighbours"][k]
    where = {}
    for i, p in enumerate(kf["point"]):
        if p >= 0 and p not in where:
            where[int(p)] = i
    i1 = [i for i, p in enumerate(cur["point"]) if int(p) in where and cur["copy_of"][i] < 0]
    return np.array(i1, "i4"), np.array([where[int(cur["point"][i])] for i in i1], "i4")


def hand_made():
    """Six pairs, one per gate, around a current keyframe at the identity and a neighbour 0.5 m to the right (the BEHIND_2 pair: 8 m
    ahead).  -> (kf1, [kf2 per pair], [expected status per pair]); every keyframe holds one feature."""
    I = _pose(np.eye(3), np.zeros(3))
    right = _pose(np.eye(3), np.array([0.5, 0.0, 0.0])); ahead = _pose(np.eye(3), np.array([0.3, 0.1, 8.0]))
    P = np.array([[0.6, 0.3, 6.0]])

    def feat(T, Xw, octave=1, du=0.0, dv=0.0):
        u, v, z = _project(T, Xw)
        return dict(x=u + du, y=v + dv, oct=np.array([octave]), desc=np.zeros((1, 32), "u1"), node=np.zeros(1), has_mp=np.zeros(1, bool),
                    point=np.zeros(1))
    cases = [
        ("LOW_PARALLAX", feat(I, P), right, feat(right, P, du=38.0)),          # the disparity of 38.2 px removed: parallel rays
        ("BEHIND_1", feat(I, P), right, feat(right, P, du=60.0)),              # past infinity: the rays meet behind both cameras
        ("BEHIND_2", feat(I, P), ahead, feat(ahead, P)),                       # through the pinhole of a camera that stands beyond the point
        ("REPROJ_1", feat(I, P, octave=0), right, feat(right, P, octave=7, dv=6.0)),
        ("REPROJ_2", feat(I, P, octave=7), right, feat(right, P, octave=0, dv=6.0)),
        ("SCALE", feat(I, P, octave=0), right, feat(right, P, octave=5)),
        ("OK", feat(I, P), right, feat(right, P)),
    ]
    return [(name, _keyframe(I, f1), _keyframe(T2, f2)) for name, f1, T2, f2 in cases]
