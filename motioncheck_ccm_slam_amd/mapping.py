"""Mirror of cslam::LocalMapping::CreateNewMapPoints (src/Mapping.cpp:284-469) over the C ABI.

One ccm_create_new_map_points call matches the current keyframe against every covisible neighbour (SearchForTriangulation without
the orientation filter), triangulates every matched pair, applies the gates of :363-448 and resolves "a feature belongs to the first
neighbour that gives it a point" on the device.  The side effects on the map (:451-466) stay with the caller, who walks the returned
list neighbour by neighbour with first[].  tap() returns what the last call stored per (neighbour, feature).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib


@dataclass
class MapKeyFrame:
    """One keyframe as CreateNewMapPoints reads it (ccm_map_keyframe)."""
    kp_x: np.ndarray            # [n] mvKeysUn[i].pt.x
    kp_y: np.ndarray
    kp_octave: np.ndarray       # [n]
    desc: np.ndarray            # [n][32] uint8
    node: np.ndarray            # [n] FeatureVector node per feature, -1 = none
    has_mp: np.ndarray          # [n] GetMapPoint(i) != null on entry
    K: np.ndarray               # fx, fy, cx, cy
    Tcw: np.ndarray             # [3][4] float32 [Rcw | tcw]
    Ow: np.ndarray              # [3] GetCameraCenter()
    scale_factors: np.ndarray   # [n_levels]
    level_sigma2: np.ndarray    # [n_levels]

    def __post_init__(self):
        a = np.ascontiguousarray
        self.kp_x, self.kp_y = a(self.kp_x, "f4").reshape(-1), a(self.kp_y, "f4").reshape(-1)
        self.kp_octave, self.node = a(self.kp_octave, "i4").reshape(-1), a(self.node, "i4").reshape(-1)
        self.desc = a(self.desc, "u1").reshape(-1, 32)
        self.has_mp = a(self.has_mp, "u1").reshape(-1)
        self.K, self.Tcw, self.Ow = a(self.K, "f4").reshape(4), a(self.Tcw, "f4").reshape(3, 4), a(self.Ow, "f4").reshape(3)
        self.scale_factors, self.level_sigma2 = a(self.scale_factors, "f4").reshape(-1), a(self.level_sigma2, "f4").reshape(-1)
        n = len(self.kp_x)
        for name in ("kp_y", "kp_octave", "desc", "node", "has_mp"):
            if len(getattr(self, name)) != n:
                raise ValueError("%s has %d rows, kp_x %d" % (name, len(getattr(self, name)), n))

    @property
    def n(self) -> int:
        return len(self.kp_x)

    def as_struct(self) -> _lib.MapKeyframe:
        p = _lib.ptr
        return _lib.MapKeyframe(self.n, p(self.kp_x), p(self.kp_y), p(self.kp_octave), p(self.desc), p(self.node), p(self.has_mp),
                                *[float(x) for x in self.K], p(self.Tcw), p(self.Ow), p(self.scale_factors), p(self.level_sigma2),
                                len(self.scale_factors))


def _mul32(*ms):
    """Product of float32 matrices, each product summed in double and stored as float32 (cv::gemm on CV_32F)."""
    out = np.asarray(ms[0], "f4")
    for m in ms[1:]:
        out = (out.astype("f8") @ np.asarray(m, "f4").astype("f8")).astype("f4")
    return out


def _kmat(K):
    return np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], "f4")


def compute_f12(kf1: MapKeyFrame, kf2: MapKeyFrame) -> np.ndarray:
    """LocalMapping::ComputeF12 (src/Mapping.cpp:549-566) in float32: K1^-T [t12]x R12 K2^-1, row-major [3][3]."""
    R1w, t1w, R2w, t2w = kf1.Tcw[:, :3], kf1.Tcw[:, 3:], kf2.Tcw[:, :3], kf2.Tcw[:, 3:]
    R12 = _mul32(R1w, R2w.T)
    t12 = (_mul32(-R1w, R2w.T, t2w) + t1w).reshape(3)
    t12x = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]], "f4")
    K1tinv = np.linalg.inv(_kmat(kf1.K).T.astype("f8")).astype("f4")
    K2inv = np.linalg.inv(_kmat(kf2.K).astype("f8")).astype("f4")
    return _mul32(K1tinv, t12x, R12, K2inv)


def compute_epipole(kf1: MapKeyFrame, kf2: MapKeyFrame) -> np.ndarray:
    """The epipole of kf1's camera centre in kf2's image (ORBmatcher.cpp:708-714), float32 (ex, ey)."""
    C2 = (_mul32(kf2.Tcw[:, :3], kf1.Ow.reshape(3, 1)) + kf2.Tcw[:, 3:]).reshape(3)
    invz = np.float32(1.0) / C2[2]
    return np.array([kf2.K[0] * C2[0] * invz + kf2.K[2], kf2.K[1] * C2[1] * invz + kf2.K[3]], "f4")


def pair_geometry(K1, Tcw1, Ow1, K2, Tcw2):
    """ccm_map_pair_geometry: (F12 [3][3], epipole [2]) float32 of the current keyframe (1) and a neighbour (2) -- the library's
    definition of ComputeF12 and the epipole.  K = (fx, fy, cx, cy)."""
    a = np.ascontiguousarray
    K1, K2 = a(K1, "f4").reshape(4), a(K2, "f4").reshape(4)
    T1, T2, O1 = a(Tcw1, "f4").reshape(12), a(Tcw2, "f4").reshape(12), a(Ow1, "f4").reshape(3)
    F = np.zeros(9, "f4"); e = np.zeros(2, "f4")
    p = _lib.ptr
    rc = _lib.load().ccm_map_pair_geometry(p(K1), p(T1), p(O1), p(K2), p(T2), p(F), p(e))
    if rc:
        raise _lib.CcmError(rc, "ccm_map_pair_geometry")
    return F.reshape(3, 3), e


def scene_median_depth(mp_id, pos, flags, Tcw):
    """ccm_scene_median_depth: (median float32, n_depths) of a keyframe whose features hold the table slots mp_id, on the table
    columns pos [capacity][3] and flags [capacity] -- KeyFrame::ComputeSceneMedianDepth(2)."""
    a = np.ascontiguousarray
    ids = a(mp_id, "i4").reshape(-1); pos = a(pos, "f4").reshape(-1, 3); flags = a(flags, "u1").reshape(-1)
    if len(flags) != len(pos):
        raise ValueError("pos has %d rows, flags %d" % (len(pos), len(flags)))
    T = a(Tcw, "f4").reshape(12)
    med = np.zeros(1, "f4"); m = np.zeros(1, "i4")
    p = _lib.ptr
    pad = lambda v: v if len(v) else np.zeros(4, v.dtype)  # noqa: E731  (an empty array may have no address)
    rc = _lib.load().ccm_scene_median_depth(len(ids), p(pad(ids)), len(pos), p(pad(pos.reshape(-1))), p(pad(flags)), p(T), p(med), p(m))
    if rc:
        raise _lib.CcmError(rc, "ccm_scene_median_depth")
    return med[0], int(m[0])


class LocalMapping:
    def __init__(self, ctx=None):
        self.ctx = ctx or _lib.default_context(0)
        self.lib = self.ctx.lib
        self._tap = None

    def CreateNewMapPoints(self, current: MapKeyFrame, neighbours, median_depth, F12=None, epipole=None, tap: bool = True):
        """-> (n_new, kf [n_new], idx1 [n_new], idx2 [n_new], x3d [n_new][3], first [n_kf + 1]).  median_depth[k] = neighbour k's
        ComputeSceneMedianDepth(2).  F12 [n_kf][3][3] / epipole [n_kf][2] default to compute_f12 / compute_epipole of the poses."""
        n_kf, n1 = len(neighbours), current.n
        if F12 is None:
            F12 = [compute_f12(current, kf) for kf in neighbours]
        if epipole is None:
            epipole = [compute_epipole(current, kf) for kf in neighbours]
        F12 = np.ascontiguousarray(F12, "f4").reshape(n_kf, 9)
        epipole = np.ascontiguousarray(epipole, "f4").reshape(n_kf, 2)
        md = np.ascontiguousarray(median_depth, "f4").reshape(-1)
        if len(md) != n_kf:
            raise ValueError("median_depth has %d entries for %d neighbours" % (len(md), n_kf))
        p = _lib.ptr
        cur = current.as_struct()
        nb = (_lib.MapKeyframe * max(n_kf, 1))(*[kf.as_struct() for kf in neighbours])
        pb = _lib.NewPointsProblem(C.pointer(cur), n_kf, nb, p(F12), p(epipole), p(md))
        rows = max(n1, 1)
        kf = np.zeros(rows, "i4"); idx1 = np.zeros(rows, "i4"); idx2 = np.zeros(rows, "i4"); x3d = np.zeros((rows, 3), "f4")
        first = np.zeros(n_kf + 1, "i4")
        res = _lib.NewPointsResult(0, p(kf), p(idx1), p(idx2), p(x3d), p(first), None)
        t = None
        if tap:
            pairs = max(n_kf * n1, 1)
            t = dict(match=np.full(pairs, -1, "i4"), status=np.zeros(pairs, "u1"), x3d_all=np.zeros((pairs, 3), "f4"))
            tp = _lib.NewPointsTap(p(t["match"]), p(t["status"]), p(t["x3d_all"]))
            res.tap = C.pointer(tp)
        n_new = self.ctx.check(self.lib.ccm_create_new_map_points(self.ctx.handle, C.byref(pb), C.byref(res)))
        self._tap = None if t is None else dict(match=t["match"][:n_kf * n1].reshape(n_kf, n1), status=t["status"][:n_kf * n1].reshape(n_kf, n1),
                                                x3d_all=t["x3d_all"][:n_kf * n1].reshape(n_kf, n1, 3))
        return n_new, kf[:n_new], idx1[:n_new], idx2[:n_new], x3d[:n_new], first

    def CreateNewMapPointsFrames(self, current, neighbours, median_depth, F12, epipole, tap: bool = True):
        """CreateNewMapPoints on keyframe handles (ccm_create_new_map_points_frames): current and neighbours are DeviceFrame objects
        with bow, camera and pose set; has_mp is map_points >= 0 as the handles hold it.  F12 [n_kf][3][3] and epipole [n_kf][2] come
        from the caller (compute_f12 / compute_epipole).  Same return tuple and tap() as CreateNewMapPoints."""
        n_kf, n1 = len(neighbours), current.n
        F12 = np.ascontiguousarray(F12, "f4").reshape(n_kf, 9)
        epipole = np.ascontiguousarray(epipole, "f4").reshape(n_kf, 2)
        md = np.ascontiguousarray(median_depth, "f4").reshape(-1)
        if len(md) != n_kf:
            raise ValueError("median_depth has %d entries for %d neighbours" % (len(md), n_kf))
        p = _lib.ptr
        nb = (C.c_void_p * max(n_kf, 1))(*[kf.handle for kf in neighbours])
        pb = _lib.NewPointsFrames(current.handle, n_kf, nb, p(F12), p(epipole), p(md))
        rows = max(n1, 1)
        kf = np.zeros(rows, "i4"); idx1 = np.zeros(rows, "i4"); idx2 = np.zeros(rows, "i4"); x3d = np.zeros((rows, 3), "f4")
        first = np.zeros(n_kf + 1, "i4")
        res = _lib.NewPointsResult(0, p(kf), p(idx1), p(idx2), p(x3d), p(first), None)
        t = None
        if tap:
            pairs = max(n_kf * n1, 1)
            t = dict(match=np.full(pairs, -1, "i4"), status=np.zeros(pairs, "u1"), x3d_all=np.zeros((pairs, 3), "f4"))
            tp = _lib.NewPointsTap(p(t["match"]), p(t["status"]), p(t["x3d_all"]))
            res.tap = C.pointer(tp)
        n_new = self.ctx.check(self.lib.ccm_create_new_map_points_frames(self.ctx.handle, C.byref(pb), C.byref(res)))
        self._tap = None if t is None else dict(match=t["match"][:n_kf * n1].reshape(n_kf, n1), status=t["status"][:n_kf * n1].reshape(n_kf, n1),
                                                x3d_all=t["x3d_all"][:n_kf * n1].reshape(n_kf, n1, 3))
        return n_new, kf[:n_new], idx1[:n_new], idx2[:n_new], x3d[:n_new], first

    def tap(self) -> dict:
        """Per (neighbour k, feature i1) of the last call: match [n_kf][n1] (index into neighbour k or -1), status [n_kf][n1]
        (_lib.NP_STATUS), x3d_all [n_kf][n1][3]."""
        if self._tap is None:
            raise RuntimeError("the last CreateNewMapPoints ran without a tap")
        return self._tap


def KeyFrameCulling(index, table, local_keys, protected_keys, thres: float, th_obs: int = 3, ctx=None, on_cull=None):
    """The loop of LocalMapping::KeyFrameCullingV3 (src/Mapping.cpp:802-862) on a covisibility.CovisibilityIndex: local_keys =
    GetVectorCovisibleKeyFrames() of the picked keyframe in its order, protected_keys = the keyframes the loop skips (mId.first 0
    or 1, :807, and mlpRecentAddedKFs, :810), thres = mfRedundancyThres.  One query covers every local keyframe that is left.  The
    verdict nRedundantObservations > mfRedundancyThres * nMPs (:857) is taken in double.  At the first keyframe that is culled the
    loop erases it from the index and calls on_cull(key): the caller's pKF->SetBadFlag() (:859) on the map.  That takes the
    keyframe's observations away, and a point left with two observers turns bad and leaves the keyframes that held it
    (src/MapPoint.cpp:494), so the caller writes such rows BAD into the table (or puts the records that changed) there; the
    keyframes behind the culled one are then queried again, since their verdicts may have changed.  Returns the culled keys in
    order."""
    from .covisibility import COVIS_REDUNDANCY
    protected = set(int(k) for k in protected_keys)
    todo = [int(k) for k in local_keys if int(k) not in protected]
    culled = []
    while todo:
        r = index.query(todo, table=table, what=COVIS_REDUNDANCY, th_obs=th_obs, ctx=ctx)
        for i, key in enumerate(todo):
            if float(r.n_redundant[i]) > float(thres) * float(r.n_mps[i]):
                index.erase(key)
                if on_cull is not None:
                    on_cull(key)
                culled.append(key)
                todo = todo[i + 1:]
                break
        else:
            todo = []
    return culled
