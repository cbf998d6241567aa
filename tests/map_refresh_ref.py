"""numpy restatement of ccm_map_table_refresh (include/ccm_hot.h): MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:929-994)
and MapPoint::UpdateNormalAndDepth (:779-823) in float32 storage with the stated float64 intermediates, and the scene the tests use.
Shared by test_map_refresh_cpu.py, test_map_refresh_gpu.py and tools/bench_map_refresh.py; nothing here touches the GPU."""
import numpy as np

F = np.float32
DESCRIPTOR, NORMAL_DEPTH = 1, 2
N_LEVELS = 8
SCALE = np.cumprod(np.concatenate([[F(1.0)], np.full(N_LEVELS - 1, F(1.2))]).astype("f4")).astype("f4")   # mvScaleFactors
SIGMA2 = (SCALE * SCALE).astype("f4")
INTR = (458.0, 457.0, 367.0, 248.0)
COUNTS = (0, 1, 2, 3, 4, 5, 8, 17, 63, 64, 65, 130, 300)          # 300: above the kernel's LDS budget of 256 rows
_POP = np.array([bin(i).count("1") for i in range(256)], "i4")


def distinctive(desc):
    """(best, tie) for the descriptors [c][32] of one point in list order: the row of the Hamming distance matrix with the least
    median, k = (int)(0.5 * (c - 1)); the first among equal medians.  tie: more than one row has the least median.  (-1, False)
    for an empty list."""
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    c = len(d)
    if c == 0:
        return -1, False
    D = _POP[d[:, None, :] ^ d[None, :, :]].sum(2)
    med = np.sort(D, axis=1)[:, int(0.5 * (c - 1))]
    return int(np.argmin(med)), int((med == med.min()).sum()) > 1


def _norm(d):
    """cv::norm of float 3-vectors [..., 3]: the squares summed in double, left to right; a double."""
    x = np.asarray(d, "f4").astype("f8")
    return np.sqrt((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])


def ray_sum(P, Ows):
    """normal = sum over the observations, in list order, of normali / cv::norm(normali) as cv::scaleAdd evaluates it:
    normal[k] = d[k] * a + normal[k] with a = (float)(1.0 / nrm), a float multiply then a float add."""
    P = np.asarray(P, "f4"); Ows = np.asarray(Ows, "f4").reshape(-1, 3)
    normal = np.zeros(3, "f4")
    with np.errstate(all="ignore"):
        for Ow in Ows:
            d = P - Ow
            a = F(1.0 / _norm(d))
            normal = (d * a).astype("f4") + normal
    return normal


def normal_depth(P, Ows, Ow_ref, level, sf=SCALE):
    """(normal [3], min_dist, max_dist) of one point with c = len(Ows) >= 1 observations."""
    P = np.asarray(P, "f4"); sf = np.asarray(sf, "f4")
    c = len(np.asarray(Ows).reshape(-1, 3))
    with np.errstate(all="ignore"):
        normal = ray_sum(P, Ows) * F(1.0 / float(c))              # Mat / n: a multiplication by the reciprocal
        dist = F(_norm(P - np.asarray(Ow_ref, "f4")))
        mx = F(dist * sf[level])
        mn = F(mx / sf[len(sf) - 1])
    return normal.astype("f4"), mn, mx


def normal_depth64(P, Ows):
    """The normal by the same formulas in float64 (the yardstick of the float32 error bound)."""
    P = np.asarray(P, "f4").astype("f8"); Ows = np.asarray(Ows, "f4").astype("f8").reshape(-1, 3)
    d = P[None, :] - Ows
    with np.errstate(all="ignore"):
        return (d / np.linalg.norm(d, axis=1)[:, None]).sum(0) / len(Ows)


def normal_depth_batch(P, Ow_kf, obs_first, obs_kf, Ow_ref, sf_level, sf_top):
    """normal_depth for many points at once, vectorised over the points and sequential over the rank of the observation (the order of
    every point's float sum is kept).  P [n][3]; Ow_kf [n_kf][3]; Ow_ref [n][3], sf_level [n] = sf_ref[level], sf_top [n] =
    sf_ref[n_levels_ref - 1] per point.  Returns (normal, min_dist, max_dist); rows of points without observations are zero."""
    P = np.asarray(P, "f4"); Ow_kf = np.asarray(Ow_kf, "f4"); first = np.asarray(obs_first); okf = np.asarray(obs_kf)
    c = np.diff(first)
    normal = np.zeros((len(c), 3), "f4")
    with np.errstate(all="ignore"):
        for r in range(int(c.max()) if len(c) else 0):
            m = np.flatnonzero(c > r)
            d = P[m] - Ow_kf[okf[first[m] + r]]
            a = (1.0 / _norm(d)).astype("f4")
            normal[m] = (d * a[:, None]).astype("f4") + normal[m]
        normal = normal * (1.0 / np.maximum(c, 1).astype("f8")).astype("f4")[:, None]
        mx = (_norm(P - np.asarray(Ow_ref, "f4")).astype("f4") * np.asarray(sf_level, "f4")).astype("f4")
        mn = (mx / np.asarray(sf_top, "f4")).astype("f4")
    return normal.astype("f4"), mn, mx


def refresh(S, rows, what=DESCRIPTOR | NORMAL_DEPTH, pos=None):
    """ccm_map_table_refresh on scene S for all its points.  rows = dict(pos, normal, min_dist, max_dist, desc) of the listed slots
    before the call, in list order; pos = the positions given in the call, or None: rows["pos"].  Returns dict(best, tie, pos, normal,
    min_dist, max_dist, desc): the rows after the call."""
    n = len(S["slot"])
    P = np.asarray(rows["pos"] if pos is None else pos, "f4")
    out = dict(best=np.full(n, -1, "i4"), tie=np.zeros(n, bool), pos=P.copy(), normal=np.array(rows["normal"], "f4"),
               min_dist=np.array(rows["min_dist"], "f4"), max_dist=np.array(rows["max_dist"], "f4"), desc=np.array(rows["desc"], np.uint8))
    kfs = S["kfs"]
    for p in range(n):
        a, b = S["obs_first"][p], S["obs_first"][p + 1]
        if a == b:
            continue
        k, f = S["obs_kf"][a:b], S["obs_feat"][a:b]
        if what & DESCRIPTOR:
            d = np.stack([kfs[ki]["desc"][fi] for ki, fi in zip(k, f)])
            out["best"][p], out["tie"][p] = distinctive(d)
            out["desc"][p] = d[out["best"][p]]
        if what & NORMAL_DEPTH:
            r = kfs[S["ref_kf"][p]]
            out["normal"][p], out["min_dist"][p], out["max_dist"][p] = normal_depth(
                P[p], np.stack([kfs[ki]["Ow"] for ki in k]), r["Ow"], r["oct"][S["ref_feat"][p]], r["sf"])
    return out


def stacked_descriptors(S):
    """(all keyframes' descriptor rows in one array, the first row of each keyframe in it)."""
    kfs = S["kfs"]
    return np.concatenate([k["desc"] for k in kfs]), np.concatenate([[0], np.cumsum([len(k["desc"]) for k in kfs])]).astype("i8")


def gathered_descriptors(S, stacked=None):
    """The old route's input: the observed descriptors gathered on the host, (desc [total][32], first [n] int64, count [n] int32)."""
    rows, base = stacked if stacked is not None else stacked_descriptors(S)
    return rows[base[S["obs_kf"]] + S["obs_feat"]], S["obs_first"][:-1].astype("i8"), np.diff(S["obs_first"]).astype("i4")


# ------------------------------------------------------------------------------------------------------------------ scene
N_KF, N_FEAT, N_POINTS, N_PROTO, CAPACITY = 8, 300, 400, 40, 1024


def scene(seed):
    """8 keyframes of 300 features whose descriptors are 40 prototypes (feature i: prototype i % 40) with 0-3 flipped bits -- a
    third of them exact copies, so that medians tie --, octaves in [0, 8), scale factors 1.2^l, camera centres in a slab 2 to 6
    units in front of the cloud (all on its -z side, so that the mean viewing direction is far from zero); 400 points in the cube
    [-0.7, 0.7]^3 that observe features of their own prototype, with every count of COUNTS (entries repeat where a count exceeds the
    features there are), in scattered slots of a table of 1024.  The reference keyframe is an entry of the list for most points and
    any feature of any keyframe for every seventh (a reference keyframe that isBad() is left out of the list).  One reference
    observation is at octave 7, one at octave 0, and point `on_centre` lies exactly on the camera centre of one of its keyframes."""
    rng = np.random.default_rng(seed)
    proto = rng.integers(0, 256, (N_PROTO, 32), dtype=np.uint8)
    kfs = []
    for k in range(N_KF):
        nflip = np.where(rng.random(N_FEAT) < 1 / 3, 0, rng.integers(1, 4, N_FEAT))
        desc = proto[np.arange(N_FEAT) % N_PROTO].copy()
        for i in range(N_FEAT):
            for b in rng.choice(256, nflip[i], replace=False):
                desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
        Ow = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-4.8, -3.0)], "f4")
        Tcw = np.concatenate([np.eye(3, dtype="f4"), -Ow[:, None]], 1).astype("f4")
        kfs.append(dict(kx=rng.uniform(0, 752, N_FEAT).astype("f4"), ky=rng.uniform(0, 480, N_FEAT).astype("f4"),
                        oct=rng.integers(0, N_LEVELS, N_FEAT).astype("i4"), desc=desc, Ow=Ow, Tcw=Tcw, sf=SCALE, sigma2=SIGMA2))
    counts = np.concatenate([COUNTS, rng.integers(0, 9, N_POINTS - len(COUNTS))]).astype("i4")
    counts = counts[rng.permutation(N_POINTS)]
    obs_first = np.concatenate([[0], np.cumsum(counts)]).astype("i4")
    obs_kf = np.zeros(obs_first[-1], "i4"); obs_feat = np.zeros(obs_first[-1], "i4")
    ref_kf = np.zeros(N_POINTS, "i4"); ref_feat = np.zeros(N_POINTS, "i4")
    for p in range(N_POINTS):
        c = counts[p]
        cand = [(k, i) for k in range(N_KF) for i in range(p % N_PROTO, N_FEAT, N_PROTO)]     # 7 or 8 features per keyframe
        pick = rng.choice(len(cand), c, replace=c > N_KF)
        for e, j in zip(range(obs_first[p], obs_first[p + 1]), pick):
            obs_kf[e], obs_feat[e] = cand[j]
        if c > 0 and p % 7 != 3:
            e = obs_first[p] + rng.integers(0, c)
            ref_kf[p], ref_feat[p] = obs_kf[e], obs_feat[e]
        else:
            ref_kf[p], ref_feat[p] = rng.integers(0, N_KF), rng.integers(0, N_FEAT)
    pos = rng.uniform(-0.7, 0.7, (N_POINTS, 3)).astype("f4")
    with_obs = np.flatnonzero(counts >= 2)
    lo, hi, on_centre = with_obs[0], with_obs[1], int(with_obs[2])
    kfs[ref_kf[lo]]["oct"][ref_feat[lo]] = 0
    kfs[ref_kf[hi]]["oct"][ref_feat[hi]] = 7
    if (ref_kf[lo], ref_feat[lo]) == (ref_kf[hi], ref_feat[hi]):
        raise ValueError("seed %d: the octave-0 and the octave-7 reference observation coincide" % seed)
    pos[on_centre] = kfs[obs_kf[obs_first[on_centre] + 1]]["Ow"]
    slot = rng.permutation(CAPACITY)[:N_POINTS].astype("i4")
    return dict(kfs=kfs, slot=slot, pos=pos, counts=counts, obs_first=obs_first, obs_kf=obs_kf, obs_feat=obs_feat, ref_kf=ref_kf,
                ref_feat=ref_feat, on_centre=on_centre, octave0=int(lo), octave7=int(hi))


def table_rows(seed, n=CAPACITY):
    """Random rows for every slot of a table (what the table holds before a refresh), flags LIVE | HAS_OBS."""
    rng = np.random.default_rng(seed)
    return dict(pos=rng.normal(0, 1, (n, 3)).astype("f4"), normal=rng.normal(0, 1, (n, 3)).astype("f4"),
                min_dist=rng.uniform(0.1, 1, n).astype("f4"), max_dist=rng.uniform(1, 9, n).astype("f4"),
                desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), flags=np.full(n, 1 | 4, np.uint8))
