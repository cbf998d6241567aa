// reloc_host.cpp -- relocalisation on frame handles and the map-point table:
//   ccm_frame_search_by_projection_keyframe   SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist), src/ORBmatcher.cpp:1478-1605
//   ccm_frame_relocalize_candidate            one candidate of ORB-SLAM's Tracking::Relocalization from the PnP pose to the verdict
// Both stage through the frame handles' block.  The search's part of it, results first:
//   [ status | match | occupied | mp_id | head | u | v | level | valid ]
// of which one download takes status .. head, or .. valid for the taps.  The queries' radius, level window, flags and descriptors stay
// in device memory (FrameState::tmm, as TrackWithMotionModel's); the id a matched feature receives is read from the keyframe's own
// mp_id.  The found set comes as a device array (an uploaded list, or the current frame's own ids).
#include "mpt_internal.h"
#include "reloc_types.h"
#include "pose_camera.h"
#include <climits>

namespace {

struct RelocIo { size_t status, out, flag, ids, head, res_end, u, v, lvl, act, tap_end; };

RelocIo reloc_layout(size_t& off, int n, int nk)
{
    RelocIo o{};
    const size_t m = (size_t)nk;
    o.status = seg(off, 16); o.out = seg(off, (size_t)n * 4); o.flag = seg(off, (size_t)n); o.ids = seg(off, (size_t)n * 4);
    o.head = seg(off, 16); o.res_end = o.head + 16;
    o.u = seg(off, m * 4); o.v = seg(off, m * 4); o.lvl = seg(off, m * 4); o.act = seg(off, m);
    o.tap_end = o.act + m;
    return o;
}

// The view as the kernel takes it; cam_dev (Tcw [12], Ow [3] in device memory) replaces p's Tcw / Ow when it is given
void reloc_view_fill(RelocArgs& A, const ccm_reloc_view* p, const float* cam_dev, float th)
{
    if (!cam_dev) { std::memcpy(A.Tcw, p->Tcw, sizeof A.Tcw); std::memcpy(A.Ow, p->Ow, sizeof A.Ow); }
    A.cam = cam_dev;
    A.fx = p->fx; A.fy = p->fy; A.cx = p->cx; A.cy = p->cy; A.min_x = p->min_x; A.max_x = p->max_x; A.min_y = p->min_y; A.max_y = p->max_y;
    A.log_scale = p->log_scale_factor; A.th = th; A.n_levels = p->n_levels;
    fill_levels(A.scale, p->scale_factors, p->n_levels);
}

// One search on a staging block the caller has reserved (o: its segments).  found_dev [n_found] is a device array; n_found < 0: every id
// cur holds now.  match and ids [N_cur] are host arrays; *bad: kf holds an id that names no LIVE slot (nothing was matched then).
// Returns n_matches or an error; one read-back and synchronisation.
int reloc_search_run(ccm_ctx* c, ccm_frame* cur, const ccm_frame* kf, ccm_map_table* t, const RelocIo& o, RelocArgs A, int orb_dist, int check_ori,
                     int n_found, const int* found_dev, bool taps, int32_t* match, int32_t* ids, int* bad)
{
    FrameState& S = *frame_state(c);
    Staging& G = S.stage;
    hipStream_t st = c->stream;
    const int n = cur->n, nk = kf->n;
    const size_t m = (size_t)nk;
    int rc;
    size_t w = 0;                                                              // device-only work area
    const size_t w_qr = seg(w, m * 4), w_minl = seg(w, m * 4), w_maxl = seg(w, m * 4), w_qflag = seg(w, m), w_qdesc = seg(w, m * 32);
    CCM_RESERVE(c, S.tmm, w + 64);
    uint8_t* wk = S.tmm.as<uint8_t>();
    int* d_head = G.dev<int>(o.head);

    CCM_HIP(c, hipMemsetAsync(d_head, 0, 16, st));
    unsigned stamp = 0;
    if ((rc = next_where_stamp(c, t, st, &stamp))) return rc;
    unsigned long long* where = t->where.as<unsigned long long>();
    if (n_found < 0) reloc_launch_mark(st, n, cur->mp_id, t->capacity, where, stamp);
    else reloc_launch_mark(st, n_found, found_dev, t->capacity, where, stamp);
    CCM_HIP(c, hipGetLastError());

    A.n_kf = nk; A.kf_id = kf->mp_id; A.where = where; A.stamp = stamp;
    A.qx = G.dev<float>(o.u); A.qy = G.dev<float>(o.v); A.level = G.dev<int>(o.lvl); A.act = G.dev<uint8_t>(o.act);
    A.qr = (float*)(wk + w_qr); A.minl = (int*)(wk + w_minl); A.maxl = (int*)(wk + w_maxl); A.qflag = wk + w_qflag; A.qdesc = wk + w_qdesc;
    A.head = d_head;
    reloc_launch_project(st, A, t->T);
    reloc_launch_clear(st, n, nk, d_head, cur->mp_id, G.dev<int>(o.out), G.dev<uint8_t>(o.flag), G.dev<int>(o.ids), A.act);
    CCM_HIP(c, hipGetLastError());

    int nm = 0;
    *bad = 0;
    if (n > 0 && nk > 0) {
        WinDevCall D{ 2, nk, A.qx, A.qy, A.qr, A.minl, A.maxl, A.qdesc, A.act, A.qflag, kf->mp_id, kf->angle, o.status, o.out, o.flag,
                      taps ? o.tap_end : o.res_end, 0.f, orb_dist, check_ori ? 1 : 0, nullptr, nullptr, nullptr, kf, G.dev<int>(o.ids), false };
        std::vector<uint8_t> occ(n);
        nm = frame_window_dev(c, cur, D, occ.data(), match);
        if (nm < 0) return nm;
        if (D.host_accept) {                                                   // nothing of the result block came down
            if ((rc = frame_fetch(c, bad, d_head, 4)) || (rc = frame_fetch(c, ids, cur->mp_id, (size_t)n * 4))) return rc;
            if (taps && ((rc = G.download(c, o.u, o.tap_end)) || (rc = G.wait(c)))) return rc;
        } else {
            G.get(bad, o.head, 4);
            G.get(ids, o.ids, (size_t)n * 4);
        }
    } else {                                                                   // no matcher: the projection's verdict and the taps alone
        if ((rc = G.download(c, o.ids, taps ? o.tap_end : o.res_end)) || (rc = G.wait(c))) return rc;
        G.get(bad, o.head, 4);
        for (int i = 0; i < n; i++) match[i] = -1;
        G.get(ids, o.ids, (size_t)n * 4);
    }
    return nm;
}

int reloc_check_view(ccm_ctx* c, const char* fn, const ccm_reloc_view* p)
{
    if (p->n_levels < 1 || p->n_levels > CCM_MAX_LEVELS) return ccm_fail(c, CCM_E_ARG, "%s: n_levels = %d outside 1..%d", fn, p->n_levels, CCM_MAX_LEVELS);
    if (!p->scale_factors) return ccm_fail(c, CCM_E_ARG, "%s: null scale_factors", fn);
    return CCM_OK;
}

}  // namespace

extern "C" {

int ccm_frame_search_by_projection_keyframe(ccm_ctx* c, ccm_frame* cur, const ccm_frame* kf, ccm_map_table* t, const ccm_reloc_view* p, float th,
                                            int orb_dist, int check_ori, int n_found, const int32_t* found, ccm_reloc_search_result* r)
{
    RoctxRange roctx_("ccm_frame_search_by_projection_keyframe");
    if (!c || !cur || !kf || !t || !p || !r) return CCM_E_ARG;
    const char* fn = "ccm_frame_search_by_projection_keyframe";
    int rc;
    if ((rc = frame_named_check(c, cur, CCM_E_STATE, fn, "cur")) || (rc = frame_named_check(c, kf, CCM_E_STATE, fn, "kf")) || (rc = check_table(c, t))) return rc;
    const bool taps = r->u != nullptr;
    if (cur == kf) return ccm_fail(c, CCM_E_ARG, "%s: cur and kf are the same handle", fn);
    if ((rc = reloc_check_view(c, fn, p))) return rc;
    if ((cur->n > 0 && (!r->match || !r->mp_id)) || (n_found > 0 && !found))
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, n_found > 0 && !found ? "found" : !r->match ? "match" : "mp_id");
    if ((r->u || r->v || r->level || r->valid) && !(r->u && r->v && r->level && r->valid))
        return ccm_fail(c, CCM_E_ARG, "%s: the taps u, v, level and valid come together", fn);
    if (check_ori && (!cur->has_angle || !kf->has_angle)) return ccm_fail(c, CCM_E_ARG, "%s: orientation check against a frame created without angles", fn);
    for (int j = 0; j < n_found; j++)
        if (found[j] < 0 || found[j] >= t->capacity) return ccm_fail(c, CCM_E_ARG, "%s: found[%d] = %d outside [0, %d)", fn, j, found[j], t->capacity);
    return table_call(c, t, false, fn, [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        Staging& G = frame_state(c)->stage;
        const int nf = n_found > 0 ? n_found : 0;
        const size_t m = (size_t)kf->n;
        r->n_matches = 0;
        size_t off = 0;
        const RelocIo o = reloc_layout(off, cur->n, kf->n);
        const size_t o_found = seg(off, (size_t)nf * 4);
        if ((rc = G.reserve(c, off))) return rc;
        G.put(o_found, found, (size_t)nf * 4);
        if ((rc = G.upload(c, o_found, o_found + (size_t)nf * 4))) return rc;    // the call's one upload: the explicit found list
        RelocArgs A{};
        reloc_view_fill(A, p, nullptr, th);
        int bad = 0;
        const int nm = reloc_search_run(c, cur, kf, t, o, A, orb_dist, check_ori, n_found < 0 ? -1 : nf, G.dev<int>(o_found), taps, r->match, r->mp_id, &bad);
        if (nm < 0) return nm;
        if (bad) return ccm_fail(c, CCM_E_ARG, "%s: kf holds a map-point id outside [0, %d) or of a slot that is not LIVE", fn, t->capacity);
        r->n_matches = nm;
        G.get(r->u, o.u, m * 4); G.get(r->v, o.v, m * 4); G.get(r->level, o.lvl, m * 4); G.get(r->valid, o.act, m);
        return CCM_OK;
    });
}

// Staging of the whole call: the search's block, then
//   [ n_inliers+status | outlier | pose7 | intr | inv_sigma2 | feature | slot | cam | backup ]
// One upload takes pose7 .. slot; every pose stage downloads n_inliers .. pose7, every search its own block.  pose7 stays in device
// memory between the stages; cam (Tcw, Ow of pose7) is made there by k_reloc_camera in front of a search.
int ccm_frame_relocalize_candidate(ccm_ctx* c, ccm_frame* cur, const ccm_frame* kf, ccm_map_table* t, const ccm_reloc_params* p, ccm_reloc_result* r)
{
    RoctxRange roctx_("ccm_frame_relocalize_candidate");
    if (!c || !cur || !kf || !t || !p || !r) return CCM_E_ARG;
    const char* fn = "ccm_frame_relocalize_candidate";
    int rc;
    if ((rc = frame_named_check(c, cur, CCM_E_STATE, fn, "cur")) || (rc = frame_named_check(c, kf, CCM_E_STATE, fn, "kf")) || (rc = check_table(c, t))) return rc;
    if (cur == kf) return ccm_fail(c, CCM_E_ARG, "%s: cur and kf are the same handle", fn);
    if ((rc = reloc_check_view(c, fn, &p->view))) return rc;
    const int n = cur->n, nm0 = p->n_matched;
    if (!p->Tcw || !p->intr || !p->inv_level_sigma2 || nm0 < 0 || (nm0 > 0 && (!p->feature || !p->slot)) || (n > 0 && (!r->mp_id || !r->outlier)))
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !p->Tcw ? "Tcw" : !p->intr ? "intr" : !p->inv_level_sigma2 ? "inv_level_sigma2" : nm0 < 0 ? "(n_matched < 0)" :
                        nm0 > 0 && (!p->feature || !p->slot) ? "feature or slot" : !r->mp_id ? "mp_id" : "outlier");
    if (p->check_ori && (!cur->has_angle || !kf->has_angle)) return ccm_fail(c, CCM_E_ARG, "%s: orientation check against a frame created without angles", fn);
    if (cur->n_levels > p->view.n_levels) return ccm_fail(c, CCM_E_ARG, "%s: octaves up to %d in cur, n_levels = %d", fn, cur->n_levels - 1, p->view.n_levels);
    for (int j = 0; j < nm0; j++) {
        if (p->feature[j] < 0 || p->feature[j] >= n) return ccm_fail(c, CCM_E_ARG, "%s: feature[%d] = %d outside [0, %d)", fn, j, p->feature[j], n);
        if (p->slot[j] < 0 || p->slot[j] >= t->capacity) return ccm_fail(c, CCM_E_ARG, "%s: slot[%d] = %d outside [0, %d)", fn, j, p->slot[j], t->capacity);
    }
    {
        std::vector<uint8_t> named(n, 0);
        for (int j = 0; j < nm0; j++) {
            if (named[p->feature[j]]) return ccm_fail(c, CCM_E_ARG, "%s: feature %d is named twice", fn, p->feature[j]);
            named[p->feature[j]] = 1;
        }
    }
    return table_call(c, t, false, fn, [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        Staging& G = frame_state(c)->stage;
        hipStream_t st = c->stream;
        const int nl = p->view.n_levels;
        r->success = 0; r->n_good = 0; r->stages = 0; r->n_add1 = 0; r->n_add2 = 0;
        if ((rc = ccm_pose_from_mat4f(p->Tcw, r->pose7))) return rc;             // Converter::toSE3Quat(mTcw)
        size_t off = 0;
        const RelocIo o = reloc_layout(off, n, kf->n);
        const size_t o_ninl = seg(off, 16), o_outl = seg(off, (size_t)n), o_pose = seg(off, 56), pose_end = o_pose + 56;
        const size_t o_intr = seg(off, 32), o_is2 = seg(off, CCM_MAX_LEVELS * 4), o_feat = seg(off, (size_t)nm0 * 4), o_slot = seg(off, (size_t)nm0 * 4);
        const size_t up_end = off;
        const size_t o_cam = seg(off, 64), o_backup = seg(off, (size_t)n * 4);
        if ((rc = G.reserve(c, off))) return rc;
        G.put(o_pose, r->pose7, 56); G.put(o_intr, p->intr, 32);
        fill_levels(G.host<float>(o_is2), p->inv_level_sigma2, nl);
        G.put(o_feat, p->feature, (size_t)nm0 * 4); G.put(o_slot, p->slot, (size_t)nm0 * 4);
        if ((rc = G.upload(c, o_pose, up_end))) return rc;

        // 1. the matches: every id -1, then the PnP inliers.  The ids on entry are kept aside until the first pose has seen the new ones.
        std::vector<int32_t> ids(n, -1), match(n);
        for (int j = 0; j < nm0; j++) ids[p->feature[j]] = p->slot[j];           // the host's copy of the handle's ids, kept through the call
        if (n > 0) CCM_HIP(c, hipMemcpyAsync(G.dev<int>(o_backup), cur->mp_id, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        if (n > 0) CCM_HIP(c, hipMemsetAsync(cur->mp_id, 0xFF, (size_t)n * 4, st));
        reloc_launch_set(st, nm0, G.dev<int>(o_feat), G.dev<int>(o_slot), n, cur->mp_id);
        CCM_HIP(c, hipGetLastError());

        const PoseIo io{ o_ninl, o_outl, o_pose, o_intr, o_is2, 0 };
        // One read-back: n_inliers, status, outlier, pose7.  discard_from: the outliers lose their id when n_inliers reaches it -- decided
        // on the device, so that nothing is queued behind the read-back (INT_MAX: they keep it).
        auto pose_stage = [&](int bit, int discard_from) -> int {
            if (n == 0) { r->n_good = 0; r->stages |= bit; return CCM_OK; }
            int e;
            if ((e = frame_pose_queue(c, cur, t->T.capacity, t->T.pos, t->T.flags, nl, io))) return e;
            if (discard_from != INT_MAX) { reloc_launch_discard(st, n, cur->mp_id, G.dev<uint8_t>(o_outl), G.dev<int>(o_ninl), discard_from); CCM_HIP(c, hipGetLastError()); }
            if ((e = G.download(c, o_ninl, pose_end)) || (e = G.wait(c))) return e;
            int head[2];
            G.get(head, o_ninl, 8);
            if (head[1]) return CCM_E_ARG;
            r->n_good = head[0]; r->stages |= bit;
            G.get(r->pose7, o_pose, 56); G.get(r->outlier, o_outl, n);
            return CCM_OK;
        };
        auto drop_outliers = [&] { for (int i = 0; i < n; i++) if (ids[i] >= 0 && r->outlier[i]) ids[i] = -1; };   // the host's copy of k_tmm_discard
        auto search_stage = [&](int bit, float th, int dist, int n_found, int32_t* n_add) -> int {
            reloc_launch_camera(st, G.dev<double>(o_pose), G.dev<float>(o_cam));
            RelocArgs A{};
            reloc_view_fill(A, &p->view, G.dev<float>(o_cam), th);
            int bad = 0;
            const int nm = reloc_search_run(c, cur, kf, t, o, A, dist, p->check_ori, n_found, G.dev<int>(o_slot), false, match.data(), ids.data(), &bad);
            if (nm < 0) return nm;
            if (bad) return ccm_fail(c, CCM_E_ARG, "%s: kf holds a map-point id outside [0, %d) or of a slot that is not LIVE", fn, t->capacity);
            *n_add = nm; r->stages |= bit;
            return CCM_OK;
        };

        auto stages = [&]() -> int {
            int e;
            // 2. the first pose; with at least min_good inliers its outliers lose their id
            if ((e = pose_stage(CCM_RELOC_POSE1, p->min_good)))
                return e != CCM_E_ARG ? e : ccm_fail(c, CCM_E_ARG, "%s: a slot that is not LIVE among the matches, or an octave of cur outside [0, %d)", fn, nl);
            if (r->n_good < p->min_good) return CCM_OK;
            drop_outliers();
            // 3. .. 6.: ORB-SLAM's nesting -- every later stage runs only when the one before it ran and passed its test
            if (r->n_good < p->enough) {
                if ((e = search_stage(CCM_RELOC_SEARCH1, p->th1, p->dist1, nm0, &r->n_add1))) return e;
                if (r->n_good + r->n_add1 >= p->enough) {
                    if ((e = pose_stage(CCM_RELOC_POSE2, INT_MAX))) return e != CCM_E_ARG ? e : ccm_fail(c, CCM_E_DEVICE, "%s: the pose stage met an id it cannot use", fn);
                    if (r->n_good > p->narrow_above && r->n_good < p->enough) {
                        if ((e = search_stage(CCM_RELOC_SEARCH2, p->th2, p->dist2, -1, &r->n_add2))) return e;
                        if (r->n_good + r->n_add2 >= p->enough) {
                            if ((e = pose_stage(CCM_RELOC_POSE3, INT_MIN))) return e != CCM_E_ARG ? e : ccm_fail(c, CCM_E_DEVICE, "%s: the pose stage met an id it cannot use", fn);
                            drop_outliers();
                        }
                    }
                }
            }
            r->success = r->n_good >= p->enough ? 1 : 0;                         // 7.
            return CCM_OK;
        };
        if ((rc = stages())) {                                                 // an error leaves the handle's ids as they were on entry
            if (n > 0 && hipMemcpyAsync(cur->mp_id, G.dev<int>(o_backup), (size_t)n * 4, hipMemcpyDeviceToDevice, st) == hipSuccess)
                (void)hipStreamSynchronize(st);
            r->success = 0;
            return rc;
        }
        if (n > 0) std::memcpy(r->mp_id, ids.data(), (size_t)n * 4);
        if (r->success) {
            float Tcw[12], Ow[3];
            ba_pose_to_camera(r->pose7, Tcw, Ow);
            if ((rc = ccm_frame_set_pose(cur, Tcw, Ow))) return rc;
        }
        return CCM_OK;
    });
}

}  // extern "C"
