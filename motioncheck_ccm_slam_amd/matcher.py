"""Host-side mirror of `cslam::ORBmatcher` (include/cslam/ORBmatcher.h:89-158) over the C ABI.

Frames / keyframes are passed as plain arrays: descriptors [N,32] uint8, the
FeatureVector as one vocabulary-node id per feature, MapPoint validity as a
0/1 mask, keypoint angles in degrees.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import BowOptions


class ORBmatcher:
    TH_HIGH = 100          # cslam/src/ORBmatcher.cpp:63-65
    TH_LOW = 50
    HISTO_LENGTH = 30

    def __init__(self, nnratio: float = 0.6, checkOri: bool = True, ctx: _lib.Context | None = None):
        self.lib = _lib.load()
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        self._ctx = ctx

    @property
    def ctx(self) -> _lib.Context:
        if self._ctx is None:
            self._ctx = _lib.default_context(0)
        return self._ctx

    @staticmethod
    def DescriptorDistance(a: np.ndarray, b: np.ndarray) -> int:
        a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
        assert a.size == 32 and b.size == 32
        return _lib.load().ccm_descriptor_distance(_lib.ptr(a), _lib.ptr(b))

    def BruteForce(self, q: np.ndarray, t: np.ndarray, nq_n=None, nt_n=None):
        """q [P,NQ,32], t [P,NT,32] -> best_idx, best_dist, second_dist, each [P,NQ] int32."""
        q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
        if q.ndim == 2:
            q = q[None]; t = t[None]
        p, nq, _ = q.shape
        nt = t.shape[1]
        bi = np.full((p, nq), -1, "i4"); bd = np.full((p, nq), 256, "i4"); sd = np.full((p, nq), 256, "i4")
        nq_n = None if nq_n is None else np.ascontiguousarray(nq_n, "i4")
        nt_n = None if nt_n is None else np.ascontiguousarray(nt_n, "i4")
        self.ctx.check(self.lib.ccm_hamming_match(self.ctx.handle, _lib.ptr(q), nq, _lib.ptr(t), nt, p,
                                                  _lib.ptr(nq_n), _lib.ptr(nt_n), _lib.ptr(bi), _lib.ptr(bd), _lib.ptr(sd)))
        return bi, bd, sd

    def RatioTest(self, best, second, th=None, strict=False):
        th = self.TH_LOW if th is None else th
        f = self.lib.ccm_ratio_test
        return np.array([f(int(b), int(s), C.c_float(self.mfNNratio), int(th), int(strict)) for b, s in zip(best, second)], bool)

    def SearchByBoW(self, desc1, node1, valid1, angle1, desc2, node2, angle2, valid2=None):
        """Both overloads of SearchByBoW: valid2=None is (KeyFrame, Frame) -- accept best <= TH_LOW;
        valid2 given is (KeyFrame, KeyFrame) -- accept best < TH_LOW.  Returns (nmatches, match12)
        with match12[i1] = index into side 2 or -1."""
        d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
        n1, n2 = len(d1), len(d2)
        node1 = np.ascontiguousarray(node1, "i4"); node2 = np.ascontiguousarray(node2, "i4")
        valid1 = np.ascontiguousarray(valid1, np.uint8)
        v2 = None if valid2 is None else np.ascontiguousarray(valid2, np.uint8)
        a1 = np.ascontiguousarray(angle1, "f4"); a2 = np.ascontiguousarray(angle2, "f4")
        opt = BowOptions(self.mfNNratio, int(self.mbCheckOrientation), self.TH_LOW, 0 if valid2 is None else 1)
        m = np.full(n1, -1, "i4")
        n = self.ctx.check(self.lib.ccm_match_bow(self.ctx.handle, C.byref(opt), _lib.ptr(d1), _lib.ptr(node1),
                                                  _lib.ptr(valid1), _lib.ptr(a1), n1, _lib.ptr(d2), _lib.ptr(node2),
                                                  _lib.ptr(v2), _lib.ptr(a2), n2, _lib.ptr(m)))
        return n, m


FRAME_GRID_COLS, FRAME_GRID_ROWS = 75, 48        # include/cslam/Frame.h:51-52


class FrameGridView:
    """What the windowed matchers need from a `Frame`: undistorted keypoints, descriptors and the feature grid
    parameters computed in the Frame constructor (src/Frame.cpp:80-88)."""

    def __init__(self, kp_x, kp_y, kp_octave, desc, min_x=0.0, max_x=752.0, min_y=0.0, max_y=480.0):
        self.kx = np.ascontiguousarray(kp_x, "f4"); self.ky = np.ascontiguousarray(kp_y, "f4")
        self.oct = np.ascontiguousarray(kp_octave, "i4"); self.desc = np.ascontiguousarray(desc, np.uint8)
        self.min_x = np.float32(min_x); self.min_y = np.float32(min_y)
        self.inv_w = np.float32(FRAME_GRID_COLS) / np.float32(np.float32(max_x) - np.float32(min_x))
        self.inv_h = np.float32(FRAME_GRID_ROWS) / np.float32(np.float32(max_y) - np.float32(min_y))

    def struct(self):
        p = _lib.ptr
        return _lib.FrameGrid(len(self.kx), p(self.kx), p(self.ky), p(self.oct), p(self.desc), float(self.min_x), float(self.min_y),
                              float(self.inv_w), float(self.inv_h), FRAME_GRID_COLS, FRAME_GRID_ROWS)


def _features_in_area(self, frame: FrameGridView, x, y, r, min_level, max_level, qdesc, cap=256):
    """Frame::GetFeaturesInArea for many queries + Hamming distance to each query descriptor."""
    x = np.ascontiguousarray(x, "f4"); y = np.ascontiguousarray(y, "f4"); r = np.ascontiguousarray(r, "f4")
    mn = np.ascontiguousarray(min_level, "i4"); mx = np.ascontiguousarray(max_level, "i4")
    qd = np.ascontiguousarray(qdesc, np.uint8)
    nq = len(x)
    ci = np.zeros((nq, cap), "i4"); cd = np.zeros((nq, cap), "i4"); cn = np.zeros(nq, "i4")
    g = frame.struct()
    self.ctx.check(self.lib.ccm_window_candidates(self.ctx.handle, C.byref(g), nq, _lib.ptr(x), _lib.ptr(y), _lib.ptr(r), _lib.ptr(mn),
                                                  _lib.ptr(mx), _lib.ptr(qd), cap, _lib.ptr(ci), _lib.ptr(cd), _lib.ptr(cn)))
    return ci, cd, cn


def _search_by_projection(self, frame: FrameGridView, scale_factors, in_view, level, view_cos, proj_x, proj_y, mp_desc,
                          mp_has_obs, occupied, th: float = 1.0):
    """ORBmatcher::SearchByProjection(Frame&, vpMapPoints, th) (ORBmatcher.cpp:71-148).
    Returns (nmatches, match[feature] = map point index or -1, occupied after the call)."""
    sf = np.ascontiguousarray(scale_factors, "f4"); iv = np.ascontiguousarray(in_view, np.uint8)
    lv = np.ascontiguousarray(level, "i4"); vc = np.ascontiguousarray(view_cos, "f4")
    px = np.ascontiguousarray(proj_x, "f4"); py = np.ascontiguousarray(proj_y, "f4")
    md = np.ascontiguousarray(mp_desc, np.uint8); ho = np.ascontiguousarray(mp_has_obs, np.uint8)
    occ = np.ascontiguousarray(occupied, np.uint8).copy()
    match = np.full(max(len(frame.kx), 1), -1, "i4")
    g = frame.struct()
    n = self.ctx.check(self.lib.ccm_search_by_projection(self.ctx.handle, C.byref(g), _lib.ptr(sf), len(iv), _lib.ptr(iv), _lib.ptr(lv),
                                                         _lib.ptr(vc), _lib.ptr(px), _lib.ptr(py), _lib.ptr(md), _lib.ptr(ho), _lib.ptr(occ),
                                                         C.c_float(th), C.c_float(self.mfNNratio), _lib.ptr(match)))
    return n, match[:len(frame.kx)], occ


ORBmatcher.FeaturesInArea = _features_in_area
ORBmatcher.SearchByProjection = _search_by_projection


def _search_by_projection_frame(self, cur: FrameGridView, cur_angle, scale_factors, valid, u, v, last_octave, last_angle, mp_desc,
                                mp_has_obs, occupied, th: float, orb_dist: int = 100):
    """ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th) (ORBmatcher.cpp:1350-1476); with
    mp_has_obs all ones and orb_dist = ORBdist also SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:1478-1605)."""
    a = np.ascontiguousarray
    ca = a(cur_angle, "f4"); sf = a(scale_factors, "f4"); va = a(valid, np.uint8); uu = a(u, "f4"); vv = a(v, "f4")
    lo = a(last_octave, "i4"); la = a(last_angle, "f4"); md = a(mp_desc, np.uint8); ho = a(mp_has_obs, np.uint8)
    occ = a(occupied, np.uint8).copy()
    match = np.full(max(len(cur.kx), 1), -1, "i4")
    g = cur.struct()
    p = _lib.ptr
    n = self.ctx.check(self.lib.ccm_search_by_projection_frame(self.ctx.handle, C.byref(g), p(ca), p(sf), len(va), p(va), p(uu), p(vv), p(lo),
                                                               p(la), p(md), p(ho), p(occ), C.c_float(th), int(self.mbCheckOrientation), int(orb_dist), p(match)))
    return n, match[:len(cur.kx)], occ


ORBmatcher.SearchByProjectionFrame = _search_by_projection_frame


def _search_by_projection_handle(self, frame, scale_factors, in_view, level, view_cos, proj_x, proj_y, mp_desc, mp_has_obs, occupied,
                                 th: float = 1.0, query_mp_id=None):
    """SearchByProjection(Frame&, vpMapPoints, th) with the frame side from a `frame.DeviceFrame` (ccm_frame_search_by_projection).
    Same results as SearchByProjection; the handle's map_points become query_mp_id[q] (or q) for every newly matched feature."""
    a = np.ascontiguousarray
    sf = a(scale_factors, "f4"); iv = a(in_view, np.uint8); lv = a(level, "i4"); vc = a(view_cos, "f4")
    px = a(proj_x, "f4"); py = a(proj_y, "f4"); md = a(mp_desc, np.uint8); ho = a(mp_has_obs, np.uint8)
    qid = None if query_mp_id is None else a(query_mp_id, "i4")
    occ = a(occupied, np.uint8).copy()
    match = np.full(max(frame.n, 1), -1, "i4")
    p = _lib.ptr
    n = self.ctx.check(self.lib.ccm_frame_search_by_projection(self.ctx.handle, C.c_void_p(frame.handle), p(sf), len(iv), p(iv), p(lv), p(vc),
                                                               p(px), p(py), p(md), p(ho), p(qid), p(occ), C.c_float(th),
                                                               C.c_float(self.mfNNratio), p(match)))
    return n, match[:frame.n], occ


def _search_by_projection_frame_handle(self, cur, last, scale_factors, valid, u, v, mp_desc, mp_has_obs, occupied, th: float,
                                       last_octave=None, last_angle=None, orb_dist: int = 100, query_mp_id=None):
    """SearchByProjection(Current, Last | KeyFrame) with `cur` a DeviceFrame (ccm_frame_search_by_projection_frame).  last = a
    DeviceFrame: its octaves, angles and map-point ids are used; last = None: the relocalisation form with last_octave /
    last_angle arrays.  Returns (nmatches, match[feature of cur] = query index or -1, occupied)."""
    a = np.ascontiguousarray
    sf = a(scale_factors, "f4"); va = a(valid, np.uint8); uu = a(u, "f4"); vv = a(v, "f4")
    md = a(mp_desc, np.uint8); ho = a(mp_has_obs, np.uint8)
    lo = None if last_octave is None else a(last_octave, "i4")
    la = None if last_angle is None else a(last_angle, "f4")
    qid = None if query_mp_id is None else a(query_mp_id, "i4")
    occ = a(occupied, np.uint8).copy()
    match = np.full(max(cur.n, 1), -1, "i4")
    p = _lib.ptr
    n = self.ctx.check(self.lib.ccm_frame_search_by_projection_frame(
        self.ctx.handle, C.c_void_p(cur.handle), None if last is None else C.c_void_p(last.handle), p(sf), len(va), p(va), p(uu), p(vv),
        p(lo), p(la), p(md), p(ho), p(qid), p(occ), C.c_float(th), int(self.mbCheckOrientation), int(orb_dist), p(match)))
    return n, match[:cur.n], occ


def _search_by_bow_handle(self, kf, frame, valid1=None, min_matches: int = 15):
    """SearchByBoW(KeyFrame, Frame) on two `frame.DeviceFrame`s that both have a bow (ccm_frame_search_by_bow).  valid1 = None: kf's
    map_points >= 0.  Returns (nmatches, match [feature of frame] = feature of kf or -1); when nmatches >= min_matches the frame's
    map_points become kf's of the matched features and -1 elsewhere (Tracking.cpp:526-529)."""
    v1 = None if valid1 is None else np.ascontiguousarray(valid1, np.uint8)
    if v1 is not None and len(v1) != kf.n:
        raise ValueError("valid1 needs %d entries" % kf.n)
    opt = BowOptions(self.mfNNratio, int(self.mbCheckOrientation), self.TH_LOW, 0)
    match = np.full(max(frame.n, 1), -1, "i4")
    n = self.ctx.check(self.lib.ccm_frame_search_by_bow(self.ctx.handle, C.c_void_p(kf.handle), C.c_void_p(frame.handle), C.byref(opt),
                                                        _lib.ptr(v1), int(min_matches), _lib.ptr(match)))
    return n, match[:frame.n]


def _search_by_bow_frames(self, kf1, kfs2, valid1=None, valid2=None):
    """SearchByBoW(KeyFrame, KeyFrame) for kf1 against every DeviceFrame of kfs2 in three launches (ccm_search_by_bow_frames).
    valid1 / valid2 (a list, one mask per candidate) = None: the handles' map_points >= 0.  Returns (nmatches [K], match12 [K][N1])."""
    K = len(kfs2)
    v1 = None if valid1 is None else np.ascontiguousarray(valid1, np.uint8)
    first2 = np.zeros(K + 1, "i4")
    for k, f in enumerate(kfs2):
        first2[k + 1] = first2[k] + f.n
    v2 = None
    if valid2 is not None:
        v2 = np.ascontiguousarray(np.concatenate([np.asarray(v, np.uint8).reshape(-1) for v in valid2]) if K else np.zeros(0), np.uint8)
        if len(v2) != first2[-1]:
            raise ValueError("valid2 needs one mask per candidate, as long as the candidate")
        if len(v2) == 0:
            v2 = np.zeros(1, np.uint8)
    opt = BowOptions(self.mfNNratio, int(self.mbCheckOrientation), self.TH_LOW, 1)
    m12 = np.full((max(K, 1), max(kf1.n, 1)), -1, "i4"); nm = np.zeros(max(K, 1), "i4")
    handles = (C.c_void_p * max(K, 1))(*[f.handle for f in kfs2])
    p = _lib.ptr
    self.ctx.check(self.lib.ccm_search_by_bow_frames(self.ctx.handle, C.c_void_p(kf1.handle), K, handles, C.byref(opt), p(v1), p(first2), p(v2),
                                                     p(m12), p(nm)))
    return nm[:K], np.ascontiguousarray(m12.reshape(-1)[:K * kf1.n].reshape(K, kf1.n))


def reloc_view(Tcw, intr, scale_factors, Ow=None, bounds=(0.0, 752.0, 0.0, 480.0), log_scale_factor=None):
    """A _lib.RelocView (ccm_reloc_view) of the current frame: Tcw 3x4 or 4x4, Ow = -Rcw^T tcw as a float cv::Mat expression when
    not given, intr = fx, fy, cx, cy, bounds = mnMinX, mnMaxX, mnMinY, mnMaxY, mfLogScaleFactor = log(mfScaleFactor) when not given.
    The structure keeps the scale factors alive."""
    from .tracking import Tracking
    T, Ow = Tracking.camera(Tcw, Ow)
    sf = np.ascontiguousarray(scale_factors, "f4")
    if log_scale_factor is None:
        log_scale_factor = np.float32(np.log(np.float64(sf[1]))) if len(sf) > 1 else np.float32(1.0)
    p = _lib.RelocView()
    p.Tcw[:] = [float(v) for v in T.reshape(-1)]; p.Ow[:] = [float(v) for v in Ow]
    p.fx, p.fy, p.cx, p.cy = [float(np.float32(v)) for v in intr]
    p.min_x, p.max_x, p.min_y, p.max_y = [float(np.float32(v)) for v in bounds]
    p.n_levels = len(sf); p.scale_factors = sf.ctypes.data; p.log_scale_factor = float(log_scale_factor)
    p._keep = sf
    return p


def _search_by_projection_keyframe_handle(self, cur, kf, table, view, th: float, orb_dist: int, found=None, taps: bool = False):
    """The relocalisation SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) on two DeviceFrames and a MapPointTable
    (ccm_frame_search_by_projection_keyframe).  view: a reloc_view; found: the slots of sAlreadyFound, or None = every id `cur` holds
    now.  Returns a dict: nmatches, match [feature of cur] = feature of kf or -1, mp_id [feature of cur] = cur's map_points after the
    call and, with taps, u / v / level / valid per feature of kf."""
    n, nk = cur.n, kf.n
    match = np.full(max(n, 1), -1, "i4"); mp_id = np.full(max(n, 1), -1, "i4")
    r = _lib.RelocSearchResult()
    r.match = match.ctypes.data; r.mp_id = mp_id.ctypes.data
    if taps:
        u = np.zeros(max(nk, 1), "f4"); v = np.zeros(max(nk, 1), "f4"); lv = np.zeros(max(nk, 1), "i4"); va = np.zeros(max(nk, 1), np.uint8)
        r.u = u.ctypes.data; r.v = v.ctypes.data; r.level = lv.ctypes.data; r.valid = va.ctypes.data
    f = None if found is None else np.ascontiguousarray(found, "i4").reshape(-1)
    self.ctx.check(self.lib.ccm_frame_search_by_projection_keyframe(
        self.ctx.handle, C.c_void_p(cur.handle), C.c_void_p(kf.handle), C.c_void_p(table.handle), C.byref(view), C.c_float(th), int(orb_dist),
        int(self.mbCheckOrientation), -1 if f is None else len(f), None if f is None or len(f) == 0 else f.ctypes.data, C.byref(r)))
    out = dict(nmatches=int(r.n_matches), match=match[:n], mp_id=mp_id[:n])
    if taps:
        out.update(u=u[:nk], v=v[:nk], level=lv[:nk], valid=va[:nk])
    return out


ORBmatcher.SearchByBoWHandle = _search_by_bow_handle
ORBmatcher.SearchByProjectionKeyFrameHandle = _search_by_projection_keyframe_handle
ORBmatcher.SearchByBoWFrames = _search_by_bow_frames
ORBmatcher.SearchByProjectionHandle = _search_by_projection_handle
ORBmatcher.SearchByProjectionFrameHandle = _search_by_projection_frame_handle


def _search_for_initialization(self, oct1, desc1, angle1, f2: FrameGridView, angle2, prev_matched, window: int = 100):
    """ORBmatcher::SearchForInitialization (ORBmatcher.cpp:448-563).  Returns (nmatches, matches12, prev_matched)."""
    a = np.ascontiguousarray
    o1 = a(oct1, "i4"); d1 = a(desc1, np.uint8); a1 = a(angle1, "f4"); a2 = a(angle2, "f4")
    pm = a(prev_matched, "f4").copy()
    m12 = np.full(max(len(o1), 1), -1, "i4")
    g = f2.struct()
    p = _lib.ptr
    n = self.ctx.check(self.lib.ccm_search_for_initialization(self.ctx.handle, len(o1), p(o1), p(d1), p(a1), C.byref(g), p(a2), p(pm), int(window),
                                                              C.c_float(self.mfNNratio), int(self.mbCheckOrientation), p(m12)))
    return n, m12[:len(o1)], pm


ORBmatcher.SearchForInitialization = _search_for_initialization


def _fuse_select(self, kf: FrameGridView, scale_factors, inv_level_sigma2, valid, u, v, level, mp_desc, th: float, chi2_check: bool,
                 accept_th: int = 50):
    """Selection loop of ORBmatcher::Fuse (both overloads).  Returns (best_idx, best_dist) per map point."""
    a = np.ascontiguousarray
    sf = a(scale_factors, "f4"); s2 = a(inv_level_sigma2, "f4"); va = a(valid, np.uint8); uu = a(u, "f4"); vv = a(v, "f4")
    lv = a(level, "i4"); md = a(mp_desc, np.uint8)
    n = len(va)
    bi = np.full(max(n, 1), -1, "i4"); bd = np.full(max(n, 1), 256, "i4")
    g = kf.struct()
    p = _lib.ptr
    self.ctx.check(self.lib.ccm_fuse_select(self.ctx.handle, C.byref(g), p(sf), p(s2), n, p(va), p(uu), p(vv), p(lv), p(md), C.c_float(th),
                                            int(chi2_check), int(accept_th), p(bi), p(bd)))
    return bi[:n], bd[:n]


ORBmatcher.FuseSelect = _fuse_select


def _fuse_select_batch(self, kfs, scale_factors, inv_level_sigma2, per_kf, th: float, chi2_check: bool, accept_th: int = 50):
    """FuseSelect for many keyframes in one launch (ccm_fuse_select_batch; the server's fuse loops, src/Mapping.cpp:515-546,
    src/MapMerger.cpp:576-586).  kfs: list of FrameGridView; per_kf: list of (valid, u, v, level, mp_desc) per keyframe.
    Returns a list of (best_idx, best_dist) per keyframe -- what FuseSelect returns keyframe by keyframe."""
    a = np.ascontiguousarray
    sf = a(scale_factors, "f4"); s2 = a(inv_level_sigma2, "f4")
    first = np.zeros(len(kfs) + 1, "i4")
    for k, t in enumerate(per_kf):
        first[k + 1] = first[k] + len(t[0])
    cat = lambda i, dt: a(np.concatenate([np.asarray(t[i]) for t in per_kf]) if len(per_kf) else np.zeros(0), dt)
    va, uu, vv, lv = cat(0, np.uint8), cat(1, "f4"), cat(2, "f4"), cat(3, "i4")
    md = a(np.concatenate([np.asarray(t[4], np.uint8).reshape(-1, 32) for t in per_kf]) if len(per_kf) else np.zeros((0, 32)), np.uint8)
    n = int(first[-1])
    bi = np.full(max(n, 1), -1, "i4"); bd = np.full(max(n, 1), 256, "i4")
    grids = (_lib.FrameGrid * max(len(kfs), 1))(*[kf.struct() for kf in kfs])
    p = _lib.ptr
    self.ctx.check(self.lib.ccm_fuse_select_batch(self.ctx.handle, len(kfs), C.cast(grids, C.c_void_p), p(sf), p(s2), p(first), p(va), p(uu), p(vv), p(lv), p(md),
                                                  C.c_float(th), int(chi2_check), int(accept_th), p(bi), p(bd)))
    return [(bi[first[k]:first[k + 1]].copy(), bd[first[k]:first[k + 1]].copy()) for k in range(len(kfs))]


ORBmatcher.FuseSelectBatch = _fuse_select_batch


def _fuse_select_batch_frames(self, frames, scale_factors, inv_level_sigma2, per_kf, th: float, chi2_check: bool, accept_th: int = 50):
    """FuseSelectBatch with the keyframes given as DeviceFrame handles (ccm_fuse_select_batch_frames): nothing of a keyframe is
    uploaded, its device-built grid is used as it is.  Returns what FuseSelectBatch returns."""
    a = np.ascontiguousarray
    sf = a(scale_factors, "f4"); s2 = a(inv_level_sigma2, "f4")
    first = np.zeros(len(frames) + 1, "i4")
    for k, t in enumerate(per_kf):
        first[k + 1] = first[k] + len(t[0])
    cat = lambda i, dt: a(np.concatenate([np.asarray(t[i]) for t in per_kf]) if len(per_kf) else np.zeros(0), dt)
    va, uu, vv, lv = cat(0, np.uint8), cat(1, "f4"), cat(2, "f4"), cat(3, "i4")
    md = a(np.concatenate([np.asarray(t[4], np.uint8).reshape(-1, 32) for t in per_kf]) if len(per_kf) else np.zeros((0, 32)), np.uint8)
    n = int(first[-1])
    bi = np.full(max(n, 1), -1, "i4"); bd = np.full(max(n, 1), 256, "i4")
    handles = (C.c_void_p * max(len(frames), 1))(*[f.handle for f in frames])
    p = _lib.ptr
    self.ctx.check(self.lib.ccm_fuse_select_batch_frames(self.ctx.handle, len(frames), handles, p(sf), p(s2), p(first), p(va), p(uu), p(vv), p(lv), p(md),
                                                         C.c_float(th), int(chi2_check), int(accept_th), p(bi), p(bd)))
    return [(bi[first[k]:first[k + 1]].copy(), bd[first[k]:first[k + 1]].copy()) for k in range(len(frames))]


ORBmatcher.FuseSelectBatchFrames = _fuse_select_batch_frames


def _fuse_select_table_frames(self, table, frames, Tcw, Ow, intr, bounds, slots, scale_factors, inv_level_sigma2=None, th: float = 3.0,
                              chi2_check: bool = True, accept_th: int = 50, skip=None, log_scale_factor=None, taps: bool = False):
    """ORBmatcher::Fuse up to the selection with the map points read from a `tracking.MapPointTable` and the keyframes given as
    DeviceFrame handles (ccm_fuse_select_table_frames): the ONE list `slots` is projected into every keyframe, gated and matched on
    the device; nothing is uploaded per pair.  Tcw [K][12] (rows of [Rcw | tcw]), Ow [K][3], intr [K][4] or [4] = fx, fy, cx, cy,
    bounds [K][4] or [4] = mnMinX, mnMaxX, mnMinY, mnMaxY.  Returns a dict of numpy arrays, each [K][len(slots)]: best_idx, best_dist
    and, with taps, gate (CCM_FG_*), u, v, level; plus n_searched."""
    a = np.ascontiguousarray
    K = len(frames)
    slot = a(slots, "i4").reshape(-1); n = len(slot)
    T = a(Tcw, "f4").reshape(K, 12); O = a(Ow, "f4").reshape(K, 3)
    I = np.broadcast_to(a(intr, "f4").reshape(-1, 4), (K, 4)); B = np.broadcast_to(a(bounds, "f4").reshape(-1, 4), (K, 4))
    sf = a(scale_factors, "f4"); s2 = None if inv_level_sigma2 is None else a(inv_level_sigma2, "f4")
    sk = None if skip is None else a(skip, np.uint8).reshape(-1)
    if sk is not None and len(sk) != n:
        raise ValueError("skip needs one entry per slot")
    if log_scale_factor is None:
        log_scale_factor = np.float32(np.log(np.float64(sf[1]))) if len(sf) > 1 else np.float32(1.0)   # mfLogScaleFactor = log(mfScaleFactor)
    views = (_lib.FuseView * max(K, 1))()
    for k, f in enumerate(frames):
        views[k].kf = f.handle
        views[k].Tcw[:] = [float(x) for x in T[k]]; views[k].Ow[:] = [float(x) for x in O[k]]
        views[k].fx, views[k].fy, views[k].cx, views[k].cy = [float(x) for x in I[k]]
        views[k].min_x, views[k].max_x, views[k].min_y, views[k].max_y = [float(x) for x in B[k]]
    pad = slot if n else np.zeros(1, "i4")
    prob = _lib.FuseTableProblem(K, views, n, _lib.ptr(pad), _lib.ptr(sk), float(log_scale_factor), len(sf), _lib.ptr(sf), _lib.ptr(s2), float(th),
                                 int(chi2_check), int(accept_th))
    m = max(K * n, 1)
    out = dict(best_idx=np.full(m, -1, "i4"), best_dist=np.full(m, 256, "i4"))
    if taps:
        out.update(gate=np.zeros(m, np.uint8), u=np.zeros(m, "f4"), v=np.zeros(m, "f4"), level=np.zeros(m, "i4"))
    g = lambda k: _lib.ptr(out[k]) if k in out else None  # noqa: E731
    res = _lib.FuseTableResult(g("best_idx"), g("best_dist"), g("gate"), g("u"), g("v"), g("level"), 0)
    self.ctx.check(self.lib.ccm_fuse_select_table_frames(self.ctx.handle, C.c_void_p(table.handle), C.byref(prob), C.byref(res)))
    ret = {k: v[:K * n].reshape(K, n) for k, v in out.items()}
    ret["n_searched"] = int(res.n_searched)
    return ret


ORBmatcher.FuseSelectTableFrames = _fuse_select_table_frames


def _log_sf(sf):
    return np.float32(np.log(np.float64(sf[1]))) if len(sf) > 1 else np.float32(1.0)   # mfLogScaleFactor = log(mfScaleFactor)


def _search_by_sim3_table_frames(self, table, pairs, scale_factors1, scale_factors2=None, th: float = 7.5, log_scale_factor1=None,
                                 log_scale_factor2=None, taps: bool = False):
    """ORBmatcher::SearchBySim3, complete, for a batch of candidate pairs with the map points read from a `tracking.MapPointTable` and
    the keyframes given as DeviceFrame handles whose map_points are table slots (ccm_search_by_sim3_table_frames).  pairs: a list of
    dicts kf1, kf2 (handles), T1w, T2w, S21, S12 ([12] or [3][4]: rows of [R | t], [sR21 | t21], [sR12 | t12]), intr (fx, fy, cx, cy of
    kf1 -- used for BOTH directions, as the reference does), bounds1, bounds2 (mnMinX, mnMaxX, mnMinY, mnMaxY), and optionally
    matched12 / matched_idx2 [N1] (default: none matched).  Returns a dict: match12 (a list of [N1] arrays), n_found (a list), total,
    and with taps gate1 / u1 / v1 / level1 / sel1 and gate2 / ... / sel2 as lists per pair."""
    a = np.ascontiguousarray
    K = len(pairs)
    sf1 = a(scale_factors1, "f4"); sf2 = sf1 if scale_factors2 is None else a(scale_factors2, "f4")
    l1 = _log_sf(sf1) if log_scale_factor1 is None else log_scale_factor1
    l2 = (_log_sf(sf2) if scale_factors2 is not None else l1) if log_scale_factor2 is None else log_scale_factor2
    recs = (_lib.Sim3SearchPair * max(K, 1))()
    keep = []
    n1 = [p["kf1"].n for p in pairs]; n2 = [p["kf2"].n for p in pairs]
    for k, p in enumerate(pairs):
        _fill_search_pair(recs[k], p, n1[k], keep)
    prob = _lib.Sim3SearchProblem(K, recs, float(th), float(l1), len(sf1), _lib.ptr(sf1), float(l2), len(sf2), _lib.ptr(sf2))
    s1, s2 = max(sum(n1), 1), max(sum(n2), 1)
    out = dict(match12=np.full(s1, -1, "i4"), n_found=np.zeros(max(K, 1), "i4"))
    if taps:
        for d, s in (("1", s1), ("2", s2)):
            out.update({"gate" + d: np.zeros(s, np.uint8), "u" + d: np.zeros(s, "f4"), "v" + d: np.zeros(s, "f4"), "level" + d: np.zeros(s, "i4"),
                        "sel" + d: np.full(s, -1, "i4")})
    g = lambda k: _lib.ptr(out[k]) if k in out else None  # noqa: E731
    res = _lib.Sim3SearchResult(*[g(k) for k in ("match12", "n_found", "gate1", "u1", "v1", "level1", "sel1", "gate2", "u2", "v2", "level2", "sel2")])
    total = self.ctx.check(self.lib.ccm_search_by_sim3_table_frames(self.ctx.handle, C.c_void_p(table.handle), C.byref(prob), C.byref(res)))
    f1 = np.concatenate([[0], np.cumsum(n1)]).astype(int); f2 = np.concatenate([[0], np.cumsum(n2)]).astype(int)
    ret = dict(total=int(total), n_found=[int(x) for x in out["n_found"][:K]])
    for k, v in out.items():
        if k != "n_found":
            f = f2 if k.endswith("2") and k != "match12" else f1
            ret[k] = [v[f[i]:f[i + 1]].copy() for i in range(K)]
    return ret


def _search_by_projection_table_frames(self, table, frames, Tcw, Ow, intr, bounds, slots, matched_slot, scale_factors, th: float = 10.0,
                                       log_scale_factor=None, taps: bool = False):
    """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) up to the acceptance with the points read from a
    `tracking.MapPointTable` and the keyframes given as DeviceFrame handles (ccm_search_by_projection_table_frames): the ONE list
    `slots` is projected into every view and accepted in list order.  Tcw [K][12], Ow [K][3], intr / bounds [K][4] or [4] as for
    FuseSelectTableFrames (the caller decomposes Scw); matched_slot: per view [N_k], vpMatched on entry as slots or -1.  Returns a dict:
    best_idx, observed ([K][n] arrays), matched_slot (a list of [N_k] arrays after the call), n_matches [K], total, and with taps gate,
    u, v, level, best_dist ([K][n])."""
    a = np.ascontiguousarray
    K = len(frames)
    slot = a(slots, "i4").reshape(-1); n = len(slot)
    T = a(Tcw, "f4").reshape(K, 12); O = a(Ow, "f4").reshape(K, 3)
    I = np.broadcast_to(a(intr, "f4").reshape(-1, 4), (K, 4)); B = np.broadcast_to(a(bounds, "f4").reshape(-1, 4), (K, 4))
    sf = a(scale_factors, "f4")
    if log_scale_factor is None:
        log_scale_factor = _log_sf(sf)
    views = (_lib.LoopView * max(K, 1))()
    ms_in = [a(ms, "i4").reshape(-1) for ms in matched_slot]
    nf = [f.n for f in frames]
    for k, f in enumerate(frames):
        if len(ms_in[k]) != nf[k]:
            raise ValueError("matched_slot needs one entry per feature of the keyframe")
        V = views[k].view
        V.kf = f.handle
        V.Tcw[:] = [float(x) for x in T[k]]; V.Ow[:] = [float(x) for x in O[k]]
        V.fx, V.fy, V.cx, V.cy = [float(x) for x in I[k]]
        V.min_x, V.max_x, V.min_y, V.max_y = [float(x) for x in B[k]]
        views[k].matched_slot = _lib.ptr(ms_in[k]) if nf[k] else None
    pad = slot if n else np.zeros(1, "i4")
    prob = _lib.LoopProjectionProblem(K, views, n, _lib.ptr(pad), float(log_scale_factor), len(sf), _lib.ptr(sf), float(th))
    m = max(K * n, 1)
    out = dict(best_idx=np.full(m, -1, "i4"), observed=np.zeros(m, np.uint8), matched_slot=np.full(max(sum(nf), 1), -1, "i4"),
               n_matches=np.zeros(max(K, 1), "i4"))
    if taps:
        out.update(gate=np.zeros(m, np.uint8), u=np.zeros(m, "f4"), v=np.zeros(m, "f4"), level=np.zeros(m, "i4"), best_dist=np.full(m, 256, "i4"))
    g = lambda k: _lib.ptr(out[k]) if k in out else None  # noqa: E731
    res = _lib.LoopProjectionResult(*[g(k) for k in ("best_idx", "observed", "matched_slot", "n_matches", "gate", "u", "v", "level", "best_dist")])
    total = self.ctx.check(self.lib.ccm_search_by_projection_table_frames(self.ctx.handle, C.c_void_p(table.handle), C.byref(prob), C.byref(res)))
    ff = np.concatenate([[0], np.cumsum(nf)]).astype(int)
    ret = {k: v[:K * n].reshape(K, n) for k, v in out.items() if k not in ("matched_slot", "n_matches")}
    ret["matched_slot"] = [out["matched_slot"][ff[k]:ff[k + 1]].copy() for k in range(K)]
    ret["n_matches"] = out["n_matches"][:K].copy()
    ret["total"] = int(total)
    return ret


def _fill_search_pair(R, p, n1, keep):
    a = np.ascontiguousarray
    R.kf1 = p["kf1"].handle; R.kf2 = p["kf2"].handle
    for name in ("T1w", "T2w", "S21", "S12"):
        getattr(R, name)[:] = [float(x) for x in a(p[name], "f4").reshape(12)]
    R.fx, R.fy, R.cx, R.cy = [float(x) for x in p["intr"]]
    R.bounds1[:] = [float(x) for x in p["bounds1"]]; R.bounds2[:] = [float(x) for x in p["bounds2"]]
    m12 = a(p.get("matched12", np.full(n1, -1)), "i4").reshape(-1); mi2 = a(p.get("matched_idx2", np.full(n1, -1)), "i4").reshape(-1)
    if len(m12) != n1 or len(mi2) != n1:
        raise ValueError("matched12 / matched_idx2 need one entry per feature of kf1")
    keep += [m12, mi2]
    R.matched12 = _lib.ptr(m12) if n1 else None; R.matched_idx2 = _lib.ptr(mi2) if n1 else None


def _compute_sim3_table_frames(self, table, pairs, scale_factors1, inv_level_sigma2_1, scale_factors2=None, inv_level_sigma2_2=None, th: float = 7.5,
                               log_scale_factor1=None, log_scale_factor2=None, taps: bool = False):
    """SearchBySim3 and OptimizeSim3 (src/LoopFinder.cpp:313-330) for a batch of candidate pairs in one call
    (ccm_compute_sim3_table_frames): the matches stay on the device, the correspondences of src/Optimizer.cpp:920-957 are listed there
    and optimised.  pairs: the dicts of SearchBySim3TableFrames -- matched12 / matched_idx2 are the solver's inliers -- plus intr2 (fx,
    fy, cx, cy of kf2; default intr), sim3 ([8] gScm: qx, qy, qz, qw, tx, ty, tz, s), fix_scale and th2.  Returns a dict: match12,
    pruned (lists of [N1] arrays), n_found, n_correspondences, n_inliers (lists), sim3 [K][8], total, and with taps the search's taps,
    corr (a list of [n][2] arrays of (i1, i2)) and inlier (a list of [n] arrays)."""
    a = np.ascontiguousarray
    K = len(pairs)
    sf1 = a(scale_factors1, "f4"); sf2 = sf1 if scale_factors2 is None else a(scale_factors2, "f4")
    is1 = a(inv_level_sigma2_1, "f4"); is2 = is1 if inv_level_sigma2_2 is None else a(inv_level_sigma2_2, "f4")
    if len(is1) != len(sf1) or len(is2) != len(sf2):
        raise ValueError("one inv_level_sigma2 per scale factor")
    l1 = _log_sf(sf1) if log_scale_factor1 is None else log_scale_factor1
    l2 = (_log_sf(sf2) if scale_factors2 is not None else l1) if log_scale_factor2 is None else log_scale_factor2
    recs = (_lib.ComputeSim3Pair * max(K, 1))()
    keep = []
    n1 = [p["kf1"].n for p in pairs]; n2 = [p["kf2"].n for p in pairs]
    for k, p in enumerate(pairs):
        _fill_search_pair(recs[k].search, p, n1[k], keep)
        recs[k].K2[:] = [float(x) for x in p.get("intr2", p["intr"])]
        recs[k].sim3[:] = [float(x) for x in a(p["sim3"], "f8").reshape(8)]
        recs[k].fix_scale = int(p.get("fix_scale", 0)); recs[k].th2 = float(p.get("th2", 10.0))
    prob = _lib.ComputeSim3Problem(K, recs, float(th), float(l1), len(sf1), _lib.ptr(sf1), _lib.ptr(is1), float(l2), len(sf2), _lib.ptr(sf2), _lib.ptr(is2))
    s1, s2 = max(sum(n1), 1), max(sum(n2), 1)
    out = dict(match12=np.full(s1, -1, "i4"), n_found=np.zeros(max(K, 1), "i4"), pruned=np.zeros(s1, np.uint8), n_correspondences=np.zeros(max(K, 1), "i4"),
               n_inliers=np.zeros(max(K, 1), "i4"), sim3=np.zeros((max(K, 1), 8), "f8"))
    if taps:
        for d, s in (("1", s1), ("2", s2)):
            out.update({"gate" + d: np.zeros(s, np.uint8), "u" + d: np.zeros(s, "f4"), "v" + d: np.zeros(s, "f4"), "level" + d: np.zeros(s, "i4"),
                        "sel" + d: np.full(s, -1, "i4")})
        out.update(corr=np.full((s1, 2), -1, "i4"), inlier=np.zeros(s1, np.uint8))
    g = lambda k: _lib.ptr(out[k]) if k in out else None  # noqa: E731
    search = _lib.Sim3SearchResult(*[g(k) for k in ("match12", "n_found", "gate1", "u1", "v1", "level1", "sel1", "gate2", "u2", "v2", "level2", "sel2")])
    res = _lib.ComputeSim3Result(search, g("pruned"), g("n_correspondences"), g("n_inliers"), g("sim3"), g("corr"), g("inlier"))
    total = self.ctx.check(self.lib.ccm_compute_sim3_table_frames(self.ctx.handle, C.c_void_p(table.handle), C.byref(prob), C.byref(res)))
    f1 = np.concatenate([[0], np.cumsum(n1)]).astype(int); f2 = np.concatenate([[0], np.cumsum(n2)]).astype(int)
    nc = out["n_correspondences"][:K]; fc = np.concatenate([[0], np.cumsum(nc)]).astype(int)
    ret = dict(total=int(total), sim3=out["sim3"][:K].copy())
    for k, v in out.items():
        if k in ("n_found", "n_correspondences", "n_inliers"):
            ret[k] = [int(x) for x in v[:K]]
        elif k in ("corr", "inlier"):
            ret[k] = [v[fc[i]:fc[i + 1]].copy() for i in range(K)]
        elif k != "sim3":
            f = f2 if k.endswith("2") and k != "match12" else f1
            ret[k] = [v[f[i]:f[i + 1]].copy() for i in range(K)]
    return ret


ORBmatcher.SearchBySim3TableFrames = _search_by_sim3_table_frames
ORBmatcher.ComputeSim3TableFrames = _compute_sim3_table_frames
ORBmatcher.SearchByProjectionTableFrames = _search_by_projection_table_frames


def _search_by_sim3(self, kf1: FrameGridView, sf1, kf2: FrameGridView, sf2, valid1, u1, v1, level1, mp_desc1, valid2, u2, v2, level2, mp_desc2,
                    th: float):
    """ORBmatcher::SearchBySim3 (ORBmatcher.cpp:1124-1348) after the caller's projections.  Returns (nFound, match12)."""
    a = np.ascontiguousarray
    arrs = [a(sf1, "f4"), a(sf2, "f4"), a(valid1, np.uint8), a(u1, "f4"), a(v1, "f4"), a(level1, "i4"), a(mp_desc1, np.uint8),
            a(valid2, np.uint8), a(u2, "f4"), a(v2, "f4"), a(level2, "i4"), a(mp_desc2, np.uint8)]
    m12 = np.full(max(len(kf1.kx), 1), -1, "i4")
    g1, g2 = kf1.struct(), kf2.struct()
    p = _lib.ptr
    n = self.ctx.check(self.lib.ccm_search_by_sim3(self.ctx.handle, C.byref(g1), p(arrs[0]), C.byref(g2), p(arrs[1]), *[p(x) for x in arrs[2:]],
                                                   C.c_float(th), p(m12)))
    return n, m12[:len(kf1.kx)]


def _search_by_projection_sim3(self, kf: FrameGridView, scale_factors, valid, u, v, level, mp_desc, observed, matched, th: float):
    """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cpp:308-446).
    Returns (nmatches, best_idx per map point, matched after the call)."""
    a = np.ascontiguousarray
    sf = a(scale_factors, "f4"); va = a(valid, np.uint8); uu = a(u, "f4"); vv = a(v, "f4"); lv = a(level, "i4"); md = a(mp_desc, np.uint8)
    ob = a(observed, np.uint8); mt = a(matched, np.uint8).copy()
    bi = np.full(max(len(va), 1), -1, "i4")
    g = kf.struct()
    p = _lib.ptr
    n = self.ctx.check(self.lib.ccm_search_by_projection_sim3(self.ctx.handle, C.byref(g), p(sf), len(va), p(va), p(uu), p(vv), p(lv), p(md), p(ob),
                                                              p(mt), C.c_float(th), p(bi)))
    return n, bi[:len(va)], mt


def _search_by_projection_sim3_batch(self, kfs, scale_factors, per_kf, th: float):
    """SearchByProjection(pKF, Scw, ...) for many keyframes in one launch per kernel (ccm_search_by_projection_sim3_batch).
    kfs: list of FrameGridView; per_kf: list of (valid, u, v, level, mp_desc, observed, matched) per keyframe.
    Returns a list of (nmatches, best_idx, matched after the call) per keyframe -- what SearchByProjectionSim3 returns keyframe by keyframe."""
    a = np.ascontiguousarray
    sf = a(scale_factors, "f4")
    K = len(kfs)
    first = np.zeros(K + 1, "i4"); ffirst = np.zeros(K + 1, "i8")
    for k, t in enumerate(per_kf):
        first[k + 1] = first[k] + len(t[0]); ffirst[k + 1] = ffirst[k] + len(kfs[k].kx)
    cat = lambda i, dt: a(np.concatenate([np.asarray(t[i]) for t in per_kf]) if K else np.zeros(0), dt)
    va, uu, vv, lv, ob = cat(0, np.uint8), cat(1, "f4"), cat(2, "f4"), cat(3, "i4"), cat(5, np.uint8)
    md = a(np.concatenate([np.asarray(t[4], np.uint8).reshape(-1, 32) for t in per_kf]) if K else np.zeros((0, 32)), np.uint8)
    mt = cat(6, np.uint8).copy()
    assert len(mt) == ffirst[-1]
    n = int(first[-1])
    bi = np.full(max(n, 1), -1, "i4"); nm = np.zeros(max(K, 1), "i4")
    if len(mt) == 0:
        mt = np.zeros(1, np.uint8)
    grids = (_lib.FrameGrid * max(K, 1))(*[kf.struct() for kf in kfs])
    p = _lib.ptr
    tot = self.ctx.check(self.lib.ccm_search_by_projection_sim3_batch(self.ctx.handle, K, C.cast(grids, C.c_void_p), p(sf), p(first), p(va), p(uu), p(vv), p(lv),
                                                                      p(md), p(ob), p(mt), C.c_float(th), p(bi), p(nm)))
    out = [(int(nm[k]), bi[first[k]:first[k + 1]].copy(), mt[ffirst[k]:ffirst[k + 1]].copy()) for k in range(K)]
    assert tot == sum(o[0] for o in out)
    return out


ORBmatcher.SearchByProjectionSim3Batch = _search_by_projection_sim3_batch


def _search_for_triangulation(self, desc1, node1, has_mp1, x1, y1, angle1, desc2, node2, has_mp2, x2, y2, angle2, octave2, F12, ex, ey,
                              scale_factors2, level_sigma2_2):
    """ORBmatcher::SearchForTriangulation (ORBmatcher.cpp:700-852).  Returns (nmatches, match12)."""
    a = np.ascontiguousarray
    d1 = a(desc1, np.uint8); n1 = a(node1, "i4"); h1 = a(has_mp1, np.uint8); xx1 = a(x1, "f4"); yy1 = a(y1, "f4"); a1 = a(angle1, "f4")
    d2 = a(desc2, np.uint8); n2 = a(node2, "i4"); h2 = a(has_mp2, np.uint8); xx2 = a(x2, "f4"); yy2 = a(y2, "f4"); a2 = a(angle2, "f4")
    o2 = a(octave2, "i4"); F = a(F12, "f4").reshape(9); sf = a(scale_factors2, "f4"); s2 = a(level_sigma2_2, "f4")
    m12 = np.full(max(len(d1), 1), -1, "i4")
    p = _lib.ptr
    n = self.ctx.check(self.lib.ccm_search_for_triangulation(self.ctx.handle, p(d1), p(n1), p(h1), p(xx1), p(yy1), p(a1), len(d1), p(d2), p(n2),
                                                             p(h2), p(xx2), p(yy2), p(a2), p(o2), len(d2), p(F), C.c_float(ex), C.c_float(ey),
                                                             p(sf), p(s2), int(self.mbCheckOrientation), p(m12)))
    return n, m12[:len(d1)]


ORBmatcher.SearchBySim3 = _search_by_sim3
ORBmatcher.SearchByProjectionSim3 = _search_by_projection_sim3
ORBmatcher.SearchForTriangulation = _search_for_triangulation
