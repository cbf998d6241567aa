"""Device-resident map-point table and the TrackLocalMap calls that work on it (include/ccm_hot.h "map-point table").

`MapPointTable` mirrors ccm_map_table: the client's map points on the GPU, one row per slot (a slot is the id a `DeviceFrame` carries
in `map_points`), updated by rows when the map changes.  `Tracking.SearchLocalPoints` is Tracking::SearchLocalPoints
(src/Tracking.cpp:860-922) in one call on a frame handle and the table; `Tracking.TrackLocalMap` adds the pose optimisation and the
inlier count of Tracking::TrackLocalMap (:623-727); `Tracking.TrackWithMotionModel` is Tracking::TrackWithMotionModel (:569-621)
behind the pose product in one call on the last and the current frame's handles and the table."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import MP_BAD, MP_HAS_OBS, MP_LIVE, MPR_DESCRIPTOR, MPR_NORMAL_DEPTH  # noqa: F401


class MapPointTable:
    """A ccm_map_table of `capacity` slots; release with `close()` (before the context goes) or use it as a context manager."""

    def __init__(self, capacity: int, ctx: _lib.Context | None = None):
        self.ctx = ctx or _lib.default_context(0)
        self.lib = self.ctx.lib
        h = C.c_void_p()
        self.ctx.check(self.lib.ccm_map_table_create(self.ctx.handle, int(capacity), C.byref(h)))
        self.handle = h.value
        self.capacity = self.lib.ccm_map_table_capacity(C.c_void_p(self.handle))

    def attach(self, ctx: _lib.Context) -> "MapPointTable":
        """A view of `ctx` on this table's rows (ccm_map_table_attach): the same methods, used with `ctx` on its own thread; the `seen`
        stamps, the visiting order and the per-call scratch are the view's own.  `close()` destroys only that handle; the rows live as
        long as any handle on them."""
        h = C.c_void_p()
        ctx.check(self.lib.ccm_map_table_attach(ctx.handle, C.c_void_p(self.handle), C.byref(h)))
        view = MapPointTable.__new__(MapPointTable)
        view.ctx = ctx; view.lib = ctx.lib; view.handle = h.value
        view.capacity = view.lib.ccm_map_table_capacity(C.c_void_p(view.handle))
        return view

    def handles(self) -> int:
        """Live handles on this table's rows (ccm_map_table_handles): 1 for a table nobody attached to, 0 once its context is gone."""
        return self.lib.ccm_map_table_handles(C.c_void_p(self.handle))

    def update(self, slot, pos=None, normal=None, min_dist=None, max_dist=None, desc=None, flags=None):
        """Write rows (ccm_map_table_update); a column left None keeps its values."""
        a = np.ascontiguousarray
        slot = a(slot, "i4"); n = len(slot)

        def col(v, t, shape):
            if v is None:
                return None
            v = a(v, t)
            if v.shape != shape:
                raise ValueError("column of shape %s, expected %s" % (v.shape, shape))
            return v
        cols = [col(pos, "f4", (n, 3)), col(normal, "f4", (n, 3)), col(min_dist, "f4", (n,)), col(max_dist, "f4", (n,)),
                col(desc, np.uint8, (n, 32)), col(flags, np.uint8, (n,))]
        u = _lib.MapUpdate(n, _lib.ptr(slot), *[_lib.ptr(c) for c in cols])
        self.ctx.check(self.lib.ccm_map_table_update(self.ctx.handle, C.c_void_p(self.handle), C.byref(u)))

    def set_order(self, slots=None):
        """The visiting order of SearchLocalPoints (ccm_map_table_set_order); None = ascending slot over the LIVE slots."""
        s = None if slots is None else np.ascontiguousarray(slots, "i4")
        pad = s if s is None or len(s) else np.zeros(1, "i4")          # an empty list still needs a non-NULL pointer
        self.ctx.check(self.lib.ccm_map_table_set_order(self.ctx.handle, C.c_void_p(self.handle), 0 if s is None else len(s), _lib.ptr(pad)))

    def fetch(self, slot):
        """Rows of `slot` as a dict of arrays (test tap, synchronises)."""
        slot = np.ascontiguousarray(slot, "i4"); n = len(slot); m = max(n, 1)
        out = dict(pos=np.zeros((m, 3), "f4"), normal=np.zeros((m, 3), "f4"), min_dist=np.zeros(m, "f4"), max_dist=np.zeros(m, "f4"),
                   desc=np.zeros((m, 32), np.uint8), flags=np.zeros(m, np.uint8), seen=np.zeros(m, "i4"))
        self.ctx.check(self.lib.ccm_map_table_fetch(self.ctx.handle, C.c_void_p(self.handle), n, _lib.ptr(slot),
                                                    *[_lib.ptr(out[k]) for k in ("pos", "normal", "min_dist", "max_dist", "desc", "flags", "seen")]))
        return {k: v[:n] for k, v in out.items()}

    def refresh(self, slot, kfs, obs_first, obs_kf, obs_feat, ref_kf=None, ref_feat=None, pos=None, flags=None, what=3, fetch=True):
        """MapPoint::ComputeDistinctiveDescriptors (what & MPR_DESCRIPTOR) and MapPoint::UpdateNormalAndDepth (what & MPR_NORMAL_DEPTH)
        for the points in `slot`, read from the keyframe handles `kfs` (DeviceFrame) and written into the table
        (ccm_map_table_refresh).  Point p observes feature obs_feat[e] of kfs[obs_kf[e]] for e in obs_first[p] .. obs_first[p+1], in the
        caller's order; ref_kf / ref_feat name its reference keyframe (needed with MPR_NORMAL_DEPTH).  pos / flags, when given, are
        written to the rows first.  Returns a dict: best [n] (the chosen observation of each list; -1 for an empty list or without
        MPR_DESCRIPTOR) and normal, min_dist, max_dist of the rows after the call; with fetch=False nothing is read back, the call does
        not synchronise and returns None."""
        a = np.ascontiguousarray
        slot = a(slot, "i4").reshape(-1); n = len(slot)
        first = a(obs_first, "i4").reshape(-1); okf = a(obs_kf, "i4").reshape(-1); ofeat = a(obs_feat, "i4").reshape(-1)
        if len(first) != n + 1 or len(okf) != len(ofeat) or (n and len(okf) < first[-1]):
            raise ValueError("obs_first needs n + 1 entries and obs_kf / obs_feat obs_first[n] each")

        def col(v, t, shape):
            if v is None:
                return None
            v = a(v, t)
            if v.shape != shape:
                raise ValueError("column of shape %s, expected %s" % (v.shape, shape))
            return v
        rkf, rfeat = col(ref_kf, "i4", (n,)), col(ref_feat, "i4", (n,))
        pos, flags = col(pos, "f4", (n, 3)), col(flags, np.uint8, (n,))
        handles = (C.c_void_p * max(len(kfs), 1))(*[k.handle for k in kfs])
        pad = lambda v: v if len(v) else np.zeros(1, v.dtype)  # noqa: E731  (an empty array may have no address)
        u = _lib.MapRefresh(n, _lib.ptr(pad(slot)), _lib.ptr(pos), _lib.ptr(flags), len(kfs), handles, _lib.ptr(first), _lib.ptr(pad(okf)),
                            _lib.ptr(pad(ofeat)), _lib.ptr(rkf), _lib.ptr(rfeat), int(what))
        if not fetch:
            self.ctx.check(self.lib.ccm_map_table_refresh(self.ctx.handle, C.c_void_p(self.handle), C.byref(u), None))
            return None
        m = max(n, 1)
        out = dict(best=np.full(m, -1, "i4"), normal=np.zeros((m, 3), "f4"), min_dist=np.zeros(m, "f4"), max_dist=np.zeros(m, "f4"))
        r = _lib.MapRefreshResult(*[_lib.ptr(out[k]) for k in ("best", "normal", "min_dist", "max_dist")])
        self.ctx.check(self.lib.ccm_map_table_refresh(self.ctx.handle, C.c_void_p(self.handle), C.byref(u), C.byref(r)))
        return {k: v[:n] for k, v in out.items()}

    def correct(self, kfs, n_moved, slot, owner, sim3_before=None, sim3_after=None, Tcw_after=None, Ow_after=None, in_order=False, lists=None,
                fetch=True):
        """The keyframe and map-point correction of a loop closure or a map merge on the table (ccm_map_table_correct_frames).
        kfs[:n_moved] (DeviceFrame) take a new pose, in the caller's iteration order; the others are only read.  Row slot[p] is moved
        by keyframe owner[p], or left exactly as it is for owner[p] == -1.  With sim3_before / sim3_after [n_moved][8] the points become
        correctedSwi.map(Siw.map(P)) and the poses [R | t/s] (MC_SIM3); with Tcw_after [n_moved][12] / Ow_after [n_moved][3] the points
        move rigidly from the handles' present poses to the given ones (MC_RIGID).  lists = (obs_first, obs_kf, obs_feat, ref_kf,
        ref_feat) as in `refresh`: UpdateNormalAndDepth on every moved point, with each keyframe's old or new camera centre as the
        reference's loop order has it -- in_order=False: every pose is set before any point (the essential-graph tail), in_order=True:
        keyframe by keyframe, the points before their keyframe's own SetPose (CorrectLoop, MergeMaps).  `DeviceFrame.pose` reports the
        new poses afterwards.  Returns a dict: pos, normal, min_dist, max_dist of the listed rows after the call; with fetch=False
        nothing is read back, the call does not synchronise and returns None."""
        a = np.ascontiguousarray
        slot = a(slot, "i4").reshape(-1); owner = a(owner, "i4").reshape(-1); n = len(slot); nm = int(n_moved)
        if len(owner) != n:
            raise ValueError("owner needs one entry per slot")
        rigid = Tcw_after is not None or Ow_after is not None
        if rigid and (sim3_before is not None or sim3_after is not None):
            raise ValueError("either the Sim3 pairs or Tcw_after / Ow_after")

        def col(v, t, shape):
            if v is None:
                return None
            v = a(v, t)
            if v.size != shape[0] * shape[1]:
                raise ValueError("array of shape %s, expected %s" % (v.shape, shape))
            return v.reshape(shape)
        pad = lambda v: v if v is None or len(v) else np.zeros(1, v.dtype)  # noqa: E731  (an empty array may have no address)
        sb, sa = pad(col(sim3_before, "f8", (nm, 8))), pad(col(sim3_after, "f8", (nm, 8)))
        Ta, Oa = pad(col(Tcw_after, "f4", (nm, 12))), pad(col(Ow_after, "f4", (nm, 3)))
        first = okf = ofeat = rkf = rfeat = None
        if lists is not None:
            first, okf, ofeat, rkf, rfeat = [a(v, "i4").reshape(-1) for v in lists]
            if len(first) != n + 1 or len(okf) != len(ofeat) or (n and len(okf) < first[-1]) or len(rkf) != n or len(rfeat) != n:
                raise ValueError("obs_first needs n + 1 entries, obs_kf / obs_feat obs_first[n] each, ref_kf / ref_feat n each")
            okf, ofeat, rkf, rfeat = pad(okf), pad(ofeat), pad(rkf), pad(rfeat)
        handles = (C.c_void_p * max(len(kfs), 1))(*[k.handle for k in kfs])
        m = max(n, 1)
        out = dict(pos=np.zeros((m, 3), "f4"), normal=np.zeros((m, 3), "f4"), min_dist=np.zeros(m, "f4"), max_dist=np.zeros(m, "f4")) if fetch else {}
        g = lambda k: _lib.ptr(out[k]) if fetch else None  # noqa: E731
        u = _lib.MapCorrect(len(kfs), handles, nm, _lib.MC_RIGID if rigid else _lib.MC_SIM3, _lib.MC_IN_ORDER if in_order else _lib.MC_POSES_FIRST,
                            _lib.ptr(sb), _lib.ptr(sa), _lib.ptr(Ta), _lib.ptr(Oa), n, _lib.ptr(pad(slot)), _lib.ptr(pad(owner)),
                            _lib.ptr(first), _lib.ptr(okf), _lib.ptr(ofeat), _lib.ptr(rkf), _lib.ptr(rfeat),
                            g("pos"), g("normal"), g("min_dist"), g("max_dist"))
        self.ctx.check(self.lib.ccm_map_table_correct_frames(self.ctx.handle, C.c_void_p(self.handle), C.byref(u)))
        return {k: v[:n] for k, v in out.items()} if fetch else None

    def close(self):
        if getattr(self, "handle", None):
            self.lib.ccm_map_table_destroy(C.c_void_p(self.handle))
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MotionModelResult:
    """What `Tracking.TrackWithMotionModel` returns (ccm_tmm_result): n_matches and passes of the search, posed, n_inliers,
    n_matches_map, pose7 (optimised when posed), match [N_cur] (feature of the last frame or -1), mp_id [N_cur] (the current frame's
    map_points after the call), outlier [N_cur] (before the discard) and, with taps, u / v / valid [N_last].  `ok` is the function's
    return value at :620, nmatchesMap >= 10, and False after the early return of :593."""
    u = v = valid = None

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def ok(self):
        return bool(self.posed) and self.n_matches_map >= 10


class Tracking:
    """The per-frame calls of Tracking::TrackLocalMap and Tracking::TrackWithMotionModel, and ORB-SLAM's Relocalization, on
    `frame.DeviceFrame`s and a `MapPointTable`."""

    @staticmethod
    def camera(Tcw, Ow=None):
        """(Tcw [12] float32 row-major 3x4, Ow [3] float32).  Ow = -Rcw^T tcw as a float cv::Mat expression (src/Frame.cpp:136)
        when not given."""
        T = np.ascontiguousarray(np.asarray(Tcw, "f4").reshape(-1)[:12].reshape(3, 4))
        if Ow is None:
            R = T[:, :3].astype("f8"); t = T[:, 3].astype("f8")
            Ow = np.array([np.float32(-np.float32(R[0, r]) * t[0] - np.float32(R[1, r]) * t[1] - np.float32(R[2, r]) * t[2]) for r in range(3)], "f4")
        return T, np.ascontiguousarray(Ow, "f4")

    @staticmethod
    def SearchLocalPoints(frame, table: MapPointTable, Tcw, intr, scale_factors, Ow=None, bounds=(0.0, 752.0, 0.0, 480.0), th=1.0, nnratio=0.8,
                          viewing_cos_limit=0.5, log_scale_factor=None, taps=False, ctx=None):
        """Tracking::SearchLocalPoints (ccm_frame_search_local_points).  intr = fx, fy, cx, cy; bounds = mnMinX, mnMaxX, mnMinY, mnMaxY.
        Returns a dict: nmatches, n_to_match, in_view_slot, match [N] (slot or -1), mp_id [N], occupied [N] and, with taps,
        proj_x / proj_y / level / view_cos per entry in view."""
        ctx = ctx or frame.ctx
        lib = _lib.load()
        T, Ow = Tracking.camera(Tcw, Ow)
        sf = np.ascontiguousarray(scale_factors, "f4")
        if log_scale_factor is None:
            log_scale_factor = np.float32(np.log(np.float64(sf[1]))) if len(sf) > 1 else np.float32(1.0)   # mfLogScaleFactor = log(mfScaleFactor)
        p = _lib.SlpParams()
        p.Tcw[:] = [float(v) for v in T.reshape(-1)]; p.Ow[:] = [float(v) for v in Ow]
        p.fx, p.fy, p.cx, p.cy = [float(np.float32(v)) for v in intr]
        p.min_x, p.max_x, p.min_y, p.max_y = [float(np.float32(v)) for v in bounds]
        p.viewing_cos_limit = float(viewing_cos_limit); p.log_scale_factor = float(log_scale_factor)
        p.n_levels = len(sf); p.scale_factors = sf.ctypes.data; p.th = float(th); p.nnratio = float(nnratio)
        n = frame.n; m = max(n, 1); cap = table.capacity
        out = dict(in_view_slot=np.zeros(cap, "i4"), match=np.full(m, -1, "i4"), mp_id=np.full(m, -1, "i4"), occupied=np.zeros(m, np.uint8))
        if taps:
            out.update(proj_x=np.zeros(cap, "f4"), proj_y=np.zeros(cap, "f4"), level=np.zeros(cap, "i4"), view_cos=np.zeros(cap, "f4"))
        g = lambda k: _lib.ptr(out[k]) if k in out else None  # noqa: E731
        r = _lib.SlpResult(0, cap, g("in_view_slot"), g("proj_x"), g("proj_y"), g("level"), g("view_cos"), g("match"), g("mp_id"), g("occupied"))
        nm = ctx.check(lib.ccm_frame_search_local_points(ctx.handle, C.c_void_p(frame.handle), C.c_void_p(table.handle), C.byref(p), C.byref(r)))
        nv = int(r.n_to_match)
        res = dict(nmatches=nm, n_to_match=nv, match=out["match"][:n], mp_id=out["mp_id"][:n], occupied=out["occupied"][:n])
        for k in ("in_view_slot", "proj_x", "proj_y", "level", "view_cos"):
            if k in out:
                res[k] = out[k][:nv]
        return res

    @staticmethod
    def PoseOptimizationTable(frame, table: MapPointTable, pose, intr, inv_level_sigma2, ctx=None):
        """Optimizer::PoseOptimizationClient(Frame&) with the points read from the table (ccm_frame_pose_optimize_table).
        Returns (pose7, outlier per feature, nInliers)."""
        ctx = ctx or frame.ctx
        lib = _lib.load()
        pose = np.ascontiguousarray(pose, "f8").copy(); intr = np.ascontiguousarray(intr, "f8")
        is2 = np.ascontiguousarray(inv_level_sigma2, "f4")
        outl = np.zeros(max(frame.n, 1), np.uint8); ninl = np.zeros(1, "i4")
        p = _lib.ptr
        ctx.check(lib.ccm_frame_pose_optimize_table(ctx.handle, C.c_void_p(frame.handle), C.c_void_p(table.handle), p(is2), len(is2), p(intr),
                                                    p(pose), p(outl), p(ninl)))
        return pose, outl[:frame.n], int(ninl[0])

    @staticmethod
    def TrackReferenceKeyFrame(frame, kf, voc, pose, intr, mp_xyz, inv_level_sigma2, nnratio=0.7, check_ori=True, min_matches=15, levelsup=4,
                               valid1=None, mp_has_obs=None, min_inliers=10, ctx=None):
        """Tracking::TrackReferenceKeyFrame (src/Tracking.cpp:514-556) on two `frame.DeviceFrame`s: ComputeBoW of the current frame
        (ccm_frame_compute_bow), SearchByBoW(reference keyframe, frame) (ccm_frame_search_by_bow; the keyframe has its bow already),
        with fewer than min_matches matches the early `return false` (:526), else PoseOptimizationClient from `pose` (the last
        frame's, :531) and "discard outliers" (:534-553): an outlier loses its map point.  mp_xyz [n_mp][3] = the positions behind
        the keyframe's map_points, mp_has_obs [n_mp] = Observations() > 0 of each (None: all).  Returns a dict: ok (nmatchesMap >=
        min_inliers, :555), nmatches, match, and after the early return nothing else; otherwise pose, outlier, n_inliers, nmatches_map and mp_id (the frame's map_points as they are left)."""
        from .matcher import ORBmatcher
        from .optimizer import Optimizer
        ctx = ctx or frame.ctx
        frame.compute_bow(voc, levelsup, outputs=False)
        nm, match = ORBmatcher(nnratio, check_ori, ctx=ctx).SearchByBoWHandle(kf, frame, valid1, min_matches)
        if nm < min_matches:
            return dict(ok=False, nmatches=nm, match=match)
        p7, outl, ninl = Optimizer.PoseOptimizationFrame(frame, pose, intr, mp_xyz, inv_level_sigma2, ctx=ctx)
        ids = frame.map_points.copy()
        has = ids >= 0
        drop = has & (outl != 0)
        if drop.any():
            ids[drop] = -1
            frame.map_points = ids
        keep = has & ~drop
        if mp_has_obs is not None:
            keep &= np.asarray(mp_has_obs, bool)[np.maximum(ids, 0)]
        nmap = int(keep.sum())
        return dict(ok=nmap >= min_inliers, nmatches=nm, match=match, pose=p7, outlier=outl, n_inliers=ninl, nmatches_map=nmap, mp_id=ids)

    @staticmethod
    def TrackWithMotionModel(cur, last, table: MapPointTable, Tcw, pose, intr, scale_factors, inv_level_sigma2, bounds=(0.0, 752.0, 0.0, 480.0),
                             th=7.0, retry_below=20, min_matches=20, check_ori=True, orb_dist=100, last_outlier=None, taps=False, ctx=None):
        """Tracking::TrackWithMotionModel (src/Tracking.cpp:569-621) behind the pose product, in one call on two `frame.DeviceFrame`s
        and the table (ccm_frame_track_motion_model): SearchByProjection(cur, last, th), once more with 2 * th when it finds fewer than
        retry_below, then -- with at least min_matches -- the pose optimisation from `pose` and "discard outliers".  Tcw = the predicted
        mVelocity * mLastFrame->mTcw (3x4 or 4x4), pose = the same as pose7, intr = fx, fy, cx, cy.  inv_level_sigma2 = None: the search
        alone.  Returns a `MotionModelResult`."""
        ctx = ctx or cur.ctx
        lib = _lib.load()
        T, _ = Tracking.camera(Tcw, np.zeros(3, "f4"))
        sf = np.ascontiguousarray(scale_factors, "f4")
        p = _lib.TmmParams()
        p.Tcw[:] = [float(v) for v in T.reshape(-1)]
        p.fx, p.fy, p.cx, p.cy = [float(np.float32(v)) for v in intr]
        p.min_x, p.max_x, p.min_y, p.max_y = [float(np.float32(v)) for v in bounds]
        p.n_levels = len(sf); p.scale_factors = sf.ctypes.data; p.th = float(th)
        p.retry_below = int(retry_below); p.min_matches = int(min_matches); p.check_ori = int(bool(check_ori)); p.orb_dist = int(orb_dist)
        lo = None if last_outlier is None else np.ascontiguousarray(last_outlier, np.uint8)
        if lo is not None and lo.shape != (last.n,):
            raise ValueError("last_outlier needs %d entries" % last.n)
        p.last_outlier = None if lo is None or last.n == 0 else lo.ctypes.data
        is2 = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, "f4")
        if is2 is not None and len(is2) != len(sf):
            raise ValueError("inv_level_sigma2 and scale_factors need one entry per level each")
        k4 = np.ascontiguousarray(intr, "f8")
        p.inv_level_sigma2 = None if is2 is None else is2.ctypes.data
        p.intr = k4.ctypes.data
        n, nl = cur.n, last.n
        match = np.full(max(n, 1), -1, "i4"); mp_id = np.full(max(n, 1), -1, "i4"); outl = np.zeros(max(n, 1), np.uint8)
        r = _lib.TmmResult()
        r.pose7[:] = [float(v) for v in np.asarray(pose, "f8").reshape(-1)[:7]]
        r.match = match.ctypes.data; r.mp_id = mp_id.ctypes.data; r.outlier = outl.ctypes.data
        if taps:
            u = np.zeros(max(nl, 1), "f4"); v = np.zeros(max(nl, 1), "f4"); valid = np.zeros(max(nl, 1), np.uint8)
            r.u = u.ctypes.data; r.v = v.ctypes.data; r.valid = valid.ctypes.data
        ctx.check(lib.ccm_frame_track_motion_model(ctx.handle, C.c_void_p(cur.handle), C.c_void_p(last.handle), C.c_void_p(table.handle),
                                                   C.byref(p), C.byref(r)))
        res = MotionModelResult(n_matches=int(r.n_matches), passes=int(r.passes), posed=bool(r.posed), n_inliers=int(r.n_inliers),
                                n_matches_map=int(r.n_matches_map), pose7=np.array(r.pose7[:], "f8"), match=match[:n], mp_id=mp_id[:n],
                                outlier=outl[:n])
        if taps:
            res.u, res.v, res.valid = u[:nl], v[:nl], valid[:nl]
        return res

    @staticmethod
    def RelocalizeCandidate(cur, kf, table: MapPointTable, Tcw, feature, slot, intr, scale_factors, inv_level_sigma2, bounds=(0.0, 752.0, 0.0, 480.0),
                            min_good=10, enough=50, narrow_above=30, th1=10.0, dist1=100, th2=3.0, dist2=64, check_ori=True, log_scale_factor=None,
                            ctx=None):
        """One relocalisation candidate from the PnP pose to the verdict (ccm_frame_relocalize_candidate): Tcw = the 4x4 float of
        PnPSolver.iterate, (feature, slot) = the PnP inliers as features of `cur` and their map points' slots.  Returns a
        `MotionModelResult`-style object: success, n_good, stages (RELOC_* bits), n_add1, n_add2, pose7, mp_id, outlier."""
        from .matcher import reloc_view
        ctx = ctx or cur.ctx
        lib = _lib.load()
        a = np.ascontiguousarray
        T = a(np.asarray(Tcw, "f4").reshape(4, 4)); ft = a(feature, "i4").reshape(-1); sl = a(slot, "i4").reshape(-1)
        if len(ft) != len(sl):
            raise ValueError("feature and slot differ in length")
        k4 = a(intr, "f8"); is2 = a(inv_level_sigma2, "f4")
        p = _lib.RelocParams()
        p.Tcw = T.ctypes.data; p.n_matched = len(ft)
        p.feature = ft.ctypes.data if len(ft) else None; p.slot = sl.ctypes.data if len(sl) else None
        p.intr = k4.ctypes.data; p.inv_level_sigma2 = is2.ctypes.data
        view = reloc_view(np.eye(4, dtype="f4"), intr, scale_factors, np.zeros(3, "f4"), bounds, log_scale_factor)
        p.view = view
        p.min_good, p.enough, p.narrow_above = int(min_good), int(enough), int(narrow_above)
        p.th1, p.dist1, p.th2, p.dist2, p.check_ori = float(th1), int(dist1), float(th2), int(dist2), int(bool(check_ori))
        n = cur.n
        mp_id = np.full(max(n, 1), -1, "i4"); outl = np.zeros(max(n, 1), np.uint8)
        r = _lib.RelocResult()
        r.mp_id = mp_id.ctypes.data; r.outlier = outl.ctypes.data
        ctx.check(lib.ccm_frame_relocalize_candidate(ctx.handle, C.c_void_p(cur.handle), C.c_void_p(kf.handle), C.c_void_p(table.handle),
                                                     C.byref(p), C.byref(r)))
        return MotionModelResult(success=bool(r.success), n_good=int(r.n_good), stages=int(r.stages), n_add1=int(r.n_add1), n_add2=int(r.n_add2),
                                 pose7=np.array(r.pose7[:], "f8"), mp_id=mp_id[:n], outlier=outl[:n])

    @staticmethod
    def Relocalization(cur, candidates, table: MapPointTable, intr, scale_factors, level_sigma2, inv_level_sigma2, draws, usable=None,
                       candidate_ids=None, min_bow_matches=15, reserve=40, ransac=(0.99, 10, 300, 4, 0.5, 5.991), ctx=None, **refine):
        """ORB-SLAM's Tracking::Relocalization on handles and the table.  `cur` has its bow (compute_bow); `candidates` are the
        keyframe handles DetectRelocalizationCandidates named (KeyFrameDatabase.DetectRelocalizationCandidates gives their keys), each
        with bow and map_points.  SearchByBoW against all of them in one call (ccm_search_by_bow_frames); a candidate with fewer than
        min_bow_matches matches is dropped; one PnPsolver per kept candidate, all created at once from the handle and the table
        (PnPSolver.from_frames) with SetRansacParameters(*ransac); then the round-robin: 5 iterations per candidate and turn, a
        candidate is dropped at bNoMore (or beyond the reserve), a pose goes through RelocalizeCandidate(**refine) and the first success
        ends the loop.  draws: the caller's random source -- an array [kept][>= maxIterations + reserve][minSet], or a callable (sizes,
        rows) -> such an array (pnpsolver.make_draws with the caller's Generator).  usable [capacity] bool: the slots that are not bad
        (None: all).  candidate_ids: the candidates' map_points when the caller has them on the host already.
        Returns a dict: success, candidate (index into candidates, or -1), result (of the successful refinement or None), n_bow [K],
        kept (the candidates that got a solver) and tried [(candidate, result)] in order."""
        from .matcher import ORBmatcher
        from .pnpsolver import PnPSolver
        ctx = ctx or cur.ctx
        K = len(candidates)
        out = dict(success=False, candidate=-1, result=None, n_bow=np.zeros(K, "i4"), kept=[], tried=[])
        if K == 0 or cur.n == 0:
            return out
        nm, m12 = ORBmatcher(0.75, True, ctx=ctx).SearchByBoWFrames(cur, candidates, valid1=np.ones(cur.n, np.uint8))
        out["n_bow"] = nm
        ids = [np.asarray(candidates[k].map_points if candidate_ids is None else candidate_ids[k], "i4") for k in range(K)]
        kept, vp, feats, slots = [], [], [], []
        for k in range(K):
            if nm[k] < min_bow_matches:
                continue
            v = np.where(m12[k] >= 0, ids[k][np.maximum(m12[k], 0)], -1).astype("i4")      # vvpMapPointMatches[k]
            f = np.flatnonzero(v >= 0)
            if usable is not None:
                f = f[np.asarray(usable, bool)[v[f]]]
            kept.append(k); vp.append(v); feats.append(f.astype("i4")); slots.append(v[f])
        out["kept"] = kept
        if not kept:
            return out
        sizes = [len(f) for f in feats]
        first = np.concatenate([[0], np.cumsum(sizes)]).astype("i4")
        rows = int(ransac[2]) + int(reserve)
        d = draws(sizes, rows) if callable(draws) else draws
        solver = PnPSolver.from_frames(cur, table, first, np.tile(np.asarray(intr, "f4").reshape(1, 4), (len(kept), 1)), np.concatenate(feats),
                                       np.concatenate(slots), level_sigma2, d, reserve=reserve, ctx=ctx)
        solver.SetRansacParameters(*ransac)
        try:
            alive = list(range(len(kept)))
            while alive and not out["success"]:
                for j in list(alive):
                    try:
                        T, no_more, inl, _ = solver.iterate(j, 5)
                    except _lib.CcmError as e:
                        if e.code != -7:                                         # CCM_E_STATE: beyond the reserve
                            raise
                        T, no_more = None, True
                    if no_more:
                        alive.remove(j)
                    if T is None:
                        continue
                    f = np.flatnonzero(inl).astype("i4")
                    res = Tracking.RelocalizeCandidate(cur, candidates[kept[j]], table, T, f, vp[j][f], intr, scale_factors, inv_level_sigma2,
                                                       ctx=ctx, **refine)
                    out["tried"].append((kept[j], res))
                    if res.success:
                        out.update(success=True, candidate=kept[j], result=res)
                        break
        finally:
            solver.close()
        return out

    @staticmethod
    def TrackLocalMap(frame, table: MapPointTable, pose, Tcw, intr, scale_factors, inv_level_sigma2, **kw):
        """Tracking::TrackLocalMap (src/Tracking.cpp:623-727) without the fork's disabled UpdateLocalMap: SearchLocalPoints, the pose
        optimisation, then mnMatchesInliers = the features that hold a map point and are no outlier (:637-648).  Returns (search result,
        pose7, outlier, mnMatchesInliers)."""
        s = Tracking.SearchLocalPoints(frame, table, Tcw, intr, scale_factors, **kw)
        p7, outl, _ = Tracking.PoseOptimizationTable(frame, table, pose, intr, inv_level_sigma2)
        inliers = int(((s["mp_id"] >= 0) & (outl == 0)).sum())
        return s, p7, outl, inliers
