"""numpy restatement of ccm_map_table_correct_frames (include/ccm_hot.h "loop and merge corrections on the table") and the scene its
tests use.  The Sim3 map and inverse are those of tests/optimizer_cases.py (correct_map_points_ref), normal and depth those of
tests/map_refresh_ref.py (normal_depth) with the rule that picks each keyframe's old or new camera centre; the rigid transform and
the new pose are restated here in float32 storage with the stated float64 intermediates.  Shared by test_map_correct_cpu.py,
test_map_correct_gpu.py and tools/bench_map_correct.py; nothing here touches the GPU."""
import numpy as np

import map_refresh_ref as R
from optimizer_cases import correct_map_points_ref, quat_R, rand_sim3

F = np.float32
SIM3, RIGID = 0, 1
POSES_FIRST, IN_ORDER = 0, 1
N_MOVED = 5
EDGE_COUNTS = (1, 63, 64, 65, 130, 300)        # observation counts on the edges of the kernel's batches of 64


def new_pose(S):
    """(Tcw [3][4], Ow [3]) float32 of a corrected Sim3 qx,qy,qz,qw,tx,ty,tz,s: the pose [R | t * (1.0 / s)] (eigt *= (1./s), then
    toCvSE3) as ccm_pose_to_camera gives it -- the rotation matrix of csrc/ba_math.h operation by operation, every entry narrowed to
    float, Ow[r] = ((-R[0][r]) * t0 - R[1][r] * t1) - R[2][r] * t2 on the widened float entries, narrowed once."""
    S = np.asarray(S, "f8")
    x, y, z, w = S[:4]
    inv = 1.0 / S[7]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    Rm = np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])
    T = np.concatenate([Rm, (S[4:7] * inv)[:, None]], 1).astype("f4")
    W = T.astype("f8")
    Ow = np.array([((-W[0, r]) * W[0, 3] - W[1, r] * W[1, 3]) - W[2, r] * W[2, 3] for r in range(3)]).astype("f4")
    return T, Ow


def sim3_positions(pos, owner, before, after):
    """Converter::toCvMat(correctedSwi.map(Siw.map(Converter::toVector3d(pos)))) for the rows with owner >= 0; the others stay."""
    return correct_map_points_ref(np.asarray(pos, "f4").astype("f8"), owner, np.asarray(before, "f8"), np.asarray(after, "f8")).astype("f4")


def rigid_positions(pos, owner, Tcw_before, Tcw_after, Ow_after):
    """Rwc * (Rcw_before * P + tcw_before) + twc as float cv::Mat expressions: each product row summed left to right in double, the
    translation added in double, narrowed to float.  Tcw_before [n_moved][3][4]: the owner handles' poses when the call is made."""
    out = np.array(pos, "f4")
    for p in np.flatnonzero(np.asarray(owner) >= 0):
        o = owner[p]
        Tb = np.asarray(Tcw_before[o], "f4").astype("f8"); Ta = np.asarray(Tcw_after[o], "f4").reshape(3, 4).astype("f8")
        Oa = np.asarray(Ow_after[o], "f4").astype("f8")
        P = out[p].astype("f8")
        Xc = np.array([F(((Tb[r, 0] * P[0] + Tb[r, 1] * P[1]) + Tb[r, 2] * P[2]) + Tb[r, 3]) for r in range(3)], "f4").astype("f8")
        out[p] = [F(((Ta[0, r] * Xc[0] + Ta[1, r] * Xc[1]) + Ta[2, r] * Xc[2]) + Oa[r]) for r in range(3)]
    return out


def camera_centre(j, owner, n_moved, order, Ow_old, Ow_new):
    """The Ow of keyframe j as UpdateNormalAndDepth of a point of keyframe `owner` finds it.  POSES_FIRST: every moved keyframe has
    its new pose.  IN_ORDER: keyframe j has it iff its SetPose came before the owner's points were refreshed, j < owner."""
    moved = j < n_moved and (order == POSES_FIRST or j < owner)
    return Ow_new[j] if moved else Ow_old[j]


def correct(C, rows, transform=SIM3, order=POSES_FIRST, lists=True, pos_after=None, n_moved=None, owner=None):
    """ccm_map_table_correct_frames on scene C (scene() below) for all its points.  rows = dict(pos, normal, min_dist, max_dist) of
    the listed slots before the call, in list order.  pos_after: positions to compute normal and depth from instead of the restated
    ones (the device's own).  Returns dict(pos, normal, min_dist, max_dist) of the rows after the call and Tcw [n_moved][3][4] /
    Ow [n_moved][3], the moved keyframes' new poses."""
    S = C["S"]; kfs = S["kfs"]
    nm = C["n_moved"] if n_moved is None else n_moved
    owner = C["owner"] if owner is None else np.asarray(owner)
    if transform == SIM3:
        poses = [new_pose(s) for s in C["sim3_after"][:nm]]
        pos = sim3_positions(rows["pos"], owner, C["sim3_before"][:max(nm, 1)], C["sim3_after"][:max(nm, 1)])
    else:
        poses = [(C["Tcw_after"][k].reshape(3, 4), C["Ow_after"][k]) for k in range(nm)]
        pos = rigid_positions(rows["pos"], owner, [k["Tcw"] for k in kfs[:nm]], C["Tcw_after"], C["Ow_after"])
    if pos_after is not None:
        pos = np.array(pos_after, "f4")
    out = dict(pos=pos, normal=np.array(rows["normal"], "f4"), min_dist=np.array(rows["min_dist"], "f4"), max_dist=np.array(rows["max_dist"], "f4"),
               Tcw=np.array([p[0] for p in poses], "f4").reshape(nm, 3, 4), Ow=np.array([p[1] for p in poses], "f4").reshape(nm, 3))
    if not lists:
        return out
    Ow_old = [k["Ow"] for k in kfs]
    for p in range(len(S["slot"])):
        a, b = S["obs_first"][p], S["obs_first"][p + 1]
        if owner[p] < 0 or a == b:
            continue
        pick = lambda j: camera_centre(j, owner[p], nm, order, Ow_old, out["Ow"])  # noqa: E731
        r = S["ref_kf"][p]
        out["normal"][p], out["min_dist"][p], out["max_dist"][p] = R.normal_depth(
            pos[p], np.stack([pick(j) for j in S["obs_kf"][a:b]]), pick(r), kfs[r]["oct"][S["ref_feat"][p]], kfs[r]["sf"])
    return out


def scene(seed=1):
    """map_refresh_ref.scene(seed) -- 8 keyframes, 400 points with every observation count of its COUNTS, capacity 1024 -- with a
    correction on top: the first N_MOVED = 5 keyframes move (three are observed but never moved), owners drawn from [0, 5) and about
    a fifth -1 (never a point with one of EDGE_COUNTS observations).  sim3_before[k] is keyframe k's pose as a Sim3 of scale 1;
    sim3_after[k] turns it by up to 0.15 rad, scales it by exp(+-0.2) and shifts its camera centre by up to 0.5 per axis, so that
    old and new camera centres differ by far more than a float's resolution.  Tcw_after / Ow_after (the rigid form) are the poses of sim3_after."""
    S = R.scene(seed)
    rng = np.random.default_rng(1000 + seed)
    n = len(S["slot"])
    owner = np.where(rng.random(n) < 0.2, -1, rng.integers(0, N_MOVED, n)).astype("i4")
    for p in np.flatnonzero(np.isin(S["counts"], EDGE_COUNTS) & (owner < 0)):      # the wave's edges belong to points that move
        owner[p] = p % N_MOVED
    before = np.zeros((N_MOVED, 8)); after = np.zeros((N_MOVED, 8))
    for k in range(N_MOVED):
        Ow = S["kfs"][k]["Ow"].astype("f8")
        before[k] = [0, 0, 0, 1, -Ow[0], -Ow[1], -Ow[2], 1]
        d = rand_sim3(rng)
        after[k, :4] = d[:4]; after[k, 7] = d[7]
        after[k, 4:7] = -d[7] * (quat_R(d[:4]) @ (Ow + rng.uniform(-0.5, 0.5, 3)))
    poses = [new_pose(s) for s in after]
    return dict(S=S, n_moved=N_MOVED, owner=owner, sim3_before=before, sim3_after=after,
                Tcw_after=np.stack([p[0].reshape(12) for p in poses]), Ow_after=np.stack([p[1] for p in poses]))


def lists(S):
    return S["obs_first"], S["obs_kf"], S["obs_feat"], S["ref_kf"], S["ref_feat"]
