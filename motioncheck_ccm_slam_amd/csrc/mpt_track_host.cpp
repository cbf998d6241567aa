// mpt_track_host.cpp -- the per-frame calls of Tracking that work on frame handles and the map-point table: SearchLocalPoints
// (src/Tracking.cpp:860-922) with its timing call, and TrackWithMotionModel (src/Tracking.cpp:569-621) at the end of this file.
//
// The calls stage through the frame handles' block (FrameState::stage, staging.h).  SearchLocalPoints
// uploads nothing: its parameters travel as kernel arguments.  Its result block is
//   [ status | match | occupied | mp_id | count | in-view slots | proj_x | proj_y | level | view_cos ]
// of which the first download takes everything up to the count, and the second, behind the matcher, the first four segments again;
// the slot list and the taps are copied at their exact length once the count is known and land with the second download.
#include "mpt_internal.h"
#include <chrono>
#include <climits>

extern "C" {

// Tracking::SearchLocalPoints, src/Tracking.cpp:860-922
int ccm_frame_search_local_points(ccm_ctx* c, ccm_frame* f, ccm_map_table* t, const ccm_slp_params* p, ccm_slp_result* r)
{
    RoctxRange roctx_("ccm_frame_search_local_points");
    if (!c || !f || !t || !p || !r) return CCM_E_ARG;
    int rc = frame_check(c, f);
    if (rc || (rc = check_table(c, t))) return rc;
    if (p->n_levels < 1 || p->n_levels > CCM_MAX_LEVELS || !p->scale_factors || r->in_view_cap < 0 || (r->in_view_cap > 0 && !r->in_view_slot) ||
        (f->n > 0 && (!r->match || !r->mp_id)))
        return ccm_fail(c, CCM_E_ARG, "bad SearchLocalPoints arguments (n_levels in 1..%d, match and mp_id of N entries)", CCM_MAX_LEVELS);
    using clk = std::chrono::steady_clock;
    const clk::time_point t_entry = clk::now();
    clk::time_point t_before, t_after;
    bool timed = false;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const int ret = table_call(c, t, false, "ccm_frame_search_local_points", [&]() -> int {    // writes the handle's own seen only
        CCM_HIP(c, hipSetDevice(c->device));
        FrameState& S = *frame_state(c);
        hipStream_t st = c->stream;
        const int n = f->n, n_order = t->order_all ? t->capacity : t->n_order, n_wg = slp_workgroups(n_order);
        const size_t m = (size_t)n_order;
        if (t->stamp == INT_MAX) { CCM_HIP(c, hipMemsetAsync(t->T.seen, 0, (size_t)t->capacity * 4, st)); t->stamp = 0; }
        const int stamp = ++t->stamp;

        size_t off = 0;
        const size_t o_status = seg(off, 16), o_out = seg(off, (size_t)n * 4), o_flag = seg(off, (size_t)n), o_ids = seg(off, (size_t)n * 4);
        const size_t res_end = o_ids + (size_t)n * 4;
        const size_t o_cnt = seg(off, 16), o_slots = seg(off, m * 4);
        const size_t first_end = o_cnt + 16;
        const size_t o_px = seg(off, m * 4), o_py = seg(off, m * 4), o_lvl = seg(off, m * 4), o_vc = seg(off, m * 4);
        Staging& G = S.stage;
        if ((rc = G.reserve(c, off))) return rc;
        size_t w = 0;                                                          // device-only work area
        const size_t w_u = seg(w, m * 4), w_v = seg(w, m * 4), w_vc = seg(w, m * 4), w_lvl = seg(w, m * 4);
        const size_t w_mask = seg(w, (size_t)n_wg * (SLP_TPB / 64) * 8), w_cnt = seg(w, (size_t)n_wg * 4), w_off = seg(w, (size_t)n_wg * 4);
        const size_t w_qr = seg(w, m * 4), w_minl = seg(w, m * 4), w_maxl = seg(w, m * 4), w_qdesc = seg(w, m * 32);
        const size_t w_act = seg(w, m), w_qflag = seg(w, m);
        CCM_RESERVE(c, S.slp, w + 64);
        uint8_t* wk = S.slp.as<uint8_t>();
        int* d_cnt = G.dev<int>(o_cnt); int* d_ids = G.dev<int>(o_ids);

        CCM_HIP(c, hipMemsetAsync(d_cnt, 0, 16, st));
        slp_launch_mark(st, t->T, n, f->mp_id, stamp, d_ids, G.dev<uint8_t>(o_flag), G.dev<int>(o_out), d_cnt);
        CCM_HIP(c, hipGetLastError());
        SlpArgs A{};
        A.n_order = n_order; A.order = t->order_all ? nullptr : t->order.as<int>(); A.stamp = stamp;
        std::memcpy(A.Tcw, p->Tcw, sizeof A.Tcw); std::memcpy(A.Ow, p->Ow, sizeof A.Ow);
        A.fx = p->fx; A.fy = p->fy; A.cx = p->cx; A.cy = p->cy; A.min_x = p->min_x; A.max_x = p->max_x; A.min_y = p->min_y; A.max_y = p->max_y;
        A.cos_limit = p->viewing_cos_limit; A.log_scale = p->log_scale_factor; A.n_levels = p->n_levels; A.th = p->th;
        fill_levels(A.scale, p->scale_factors, p->n_levels);
        A.tmp_u = (float*)(wk + w_u); A.tmp_v = (float*)(wk + w_v); A.tmp_vc = (float*)(wk + w_vc); A.tmp_level = (int*)(wk + w_lvl);
        A.mask = (unsigned long long*)(wk + w_mask); A.wg_cnt = (int*)(wk + w_cnt); A.wg_off = (int*)(wk + w_off);
        A.qx = G.dev<float>(o_px); A.qy = G.dev<float>(o_py); A.qr = (float*)(wk + w_qr); A.minl = (int*)(wk + w_minl); A.maxl = (int*)(wk + w_maxl);
        A.qdesc = wk + w_qdesc; A.qact = wk + w_act; A.qflag = wk + w_qflag; A.slots = G.dev<int>(o_slots);
        A.tap_level = G.dev<int>(o_lvl); A.tap_vc = G.dev<float>(o_vc);
        slp_launch_frustum(st, A, t->T, d_cnt);
        CCM_HIP(c, hipGetLastError());
        t_before = clk::now();
        if ((rc = G.download(c, 0, first_end)) || (rc = G.wait(c))) return rc; // the count (16 bytes) behind the first loop's results
        t_after = clk::now(); timed = true;

        int head[2];
        G.get(head, o_cnt, 8);
        const int nv = head[0];
        if (head[1]) return ccm_fail(c, CCM_E_ARG, "the frame holds a map-point id outside [0, %d) or of a slot that is not LIVE", t->capacity);
        if (nv < 0 || nv > n_order) return ccm_fail(c, CCM_E_DEVICE, "%d entries in view of %d", nv, n_order);
        r->n_to_match = nv;
        if (nv > r->in_view_cap) return ccm_fail(c, CCM_E_CAPACITY, "%d map points in view, room for %d", nv, r->in_view_cap);
        if (n > 0) CCM_HIP(c, hipMemcpyAsync(f->mp_id, d_ids, (size_t)n * 4, hipMemcpyDeviceToDevice, st));   // the bad ones cleared
        const bool taps = r->proj_x || r->proj_y || r->level || r->view_cos;
        if (nv == 0 || n == 0) {                                               // :910: no matcher
            for (int i = 0; i < n; i++) r->match[i] = -1;
            G.get(r->mp_id, o_ids, (size_t)n * 4);
            G.get(r->occupied, o_flag, n);
            if (nv == 0) return 0;
            if ((rc = G.download(c, o_slots, o_slots + (size_t)nv * 4)) || (rc = G.wait(c))) return rc;    // an empty frame: the slot list alone
            if (taps && ((rc = G.download(c, o_px, o_vc + (size_t)nv * 4)) || (rc = G.wait(c)))) return rc;
        } else {                                                               // exact lengths; they land before the matcher's download
            if ((rc = G.download(c, o_slots, o_slots + (size_t)nv * 4))) return rc;
            if (taps)
                for (size_t o : { o_px, o_py, o_lvl, o_vc }) if ((rc = G.download(c, o, o + (size_t)nv * 4))) return rc;
        }
        int nmatches = 0;
        if (nv > 0 && n > 0) {
            WinDevCall D{ 0, nv, A.qx, A.qy, A.qr, A.minl, A.maxl, A.qdesc, A.qact, A.qflag, A.slots, nullptr, o_status, o_out, o_flag, res_end,
                          p->nnratio, 0, 0, nullptr, nullptr, nullptr, nullptr, d_ids, false };
            std::vector<uint8_t> occ_tmp;
            uint8_t* occ = r->occupied;
            if (!occ) { occ_tmp.resize(n); occ = occ_tmp.data(); }
            nmatches = frame_window_dev(c, f, D, occ, r->match);
            if (nmatches < 0) return nmatches;
            if (D.host_accept) { if ((rc = frame_fetch(c, r->mp_id, f->mp_id, (size_t)n * 4))) return rc; }
            else G.get(r->mp_id, o_ids, (size_t)n * 4);
            G.get(r->in_view_slot, o_slots, (size_t)nv * 4);
            for (int i = 0; i < n; i++) if (r->match[i] >= 0) r->match[i] = r->in_view_slot[r->match[i]];   // query -> slot
        }
        if (n == 0) G.get(r->in_view_slot, o_slots, (size_t)nv * 4);
        G.get(r->proj_x, o_px, (size_t)nv * 4); G.get(r->proj_y, o_py, (size_t)nv * 4);
        G.get(r->level, o_lvl, (size_t)nv * 4); G.get(r->view_cos, o_vc, (size_t)nv * 4);
        return nmatches;
    });
    if (timed) {
        double* t_ms = c->frame->slp_ms;
        t_ms[0] = ms(t_entry, t_before); t_ms[1] = ms(t_before, t_after); t_ms[2] = ms(t_after, clk::now());
    }
    return ret;
}

int ccm_frame_search_local_points_timing(ccm_ctx* c, double out[3])
{
    if (!c || !out) return CCM_E_ARG;
    if (!c->frame || c->frame->slp_ms[0] < 0) return ccm_fail(c, CCM_E_STATE, "no ccm_frame_search_local_points on this context yet");
    std::memcpy(out, c->frame->slp_ms, sizeof c->frame->slp_ms);
    return CCM_OK;
}

// Tracking::TrackWithMotionModel behind the pose product, src/Tracking.cpp:579-621.  Staging, results first:
//   [ status | match | occupied | last_outlier | head | pose7 | intr | inv_sigma2 | scale | n_inliers | outlier | mp_id | u | v | valid ]
// One upload takes last_outlier .. scale (head as zeros); every pass downloads status .. head, the end of the call head .. mp_id, or
// .. valid for the taps.  The queries' radius, level window, HAS_OBS flags and descriptors stay in device memory (FrameState::tmm);
// the id a matched feature receives is read from last's own mp_id (a query's slot is its feature's id), so no id list is made.
int ccm_frame_track_motion_model(ccm_ctx* c, ccm_frame* cur, const ccm_frame* last, ccm_map_table* t, const ccm_tmm_params* p, ccm_tmm_result* r)
{
    RoctxRange roctx_("ccm_frame_track_motion_model");
    if (!c || !cur || !last || !t || !p || !r) return CCM_E_ARG;
    const char* fn = "ccm_frame_track_motion_model";
    int rc;
    if ((rc = frame_named_check(c, cur, CCM_E_STATE, fn, "cur")) || (rc = frame_named_check(c, last, CCM_E_STATE, fn, "last")) || (rc = check_table(c, t))) return rc;
    const bool pose = p->inv_level_sigma2 != nullptr, taps = r->u != nullptr;
    if (cur == last) return ccm_fail(c, CCM_E_ARG, "%s: cur and last are the same handle", fn);
    if (p->n_levels < 1 || p->n_levels > CCM_MAX_LEVELS) return ccm_fail(c, CCM_E_ARG, "%s: n_levels = %d outside 1..%d", fn, p->n_levels, CCM_MAX_LEVELS);
    if (!p->scale_factors || (pose && !p->intr) || (cur->n > 0 && (!r->match || !r->mp_id || !r->outlier)))
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !p->scale_factors ? "scale_factors" : pose && !p->intr ? "intr with inv_level_sigma2" :
                        !r->match ? "match" : !r->mp_id ? "mp_id" : "outlier");
    if ((r->u || r->v || r->valid) && !(r->u && r->v && r->valid)) return ccm_fail(c, CCM_E_ARG, "%s: the taps u, v and valid come together", fn);
    if (p->check_ori && (!cur->has_angle || !last->has_angle)) return ccm_fail(c, CCM_E_ARG, "%s: orientation check against a frame created without angles", fn);
    if (last->n_levels > p->n_levels || (pose && cur->n_levels > p->n_levels))
        return ccm_fail(c, CCM_E_ARG, "%s: octaves up to %d in %s, n_levels = %d", fn, (last->n_levels > p->n_levels ? last : cur)->n_levels - 1,
                        last->n_levels > p->n_levels ? "last" : "cur", p->n_levels);
    return table_call(c, t, false, fn, [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        FrameState& S = *frame_state(c);
        hipStream_t st = c->stream;
        const int n = cur->n, nl = last->n;
        r->n_matches = 0; r->passes = 0; r->posed = 0; r->n_inliers = 0; r->n_matches_map = 0;
        if (n == 0 || nl == 0) {                                               // :579 still happens; no matcher, no pose
            if (n > 0) {
                CCM_HIP(c, hipMemsetAsync(cur->mp_id, 0xFF, (size_t)n * 4, st));
                for (int i = 0; i < n; i++) { r->match[i] = -1; r->mp_id[i] = -1; }
                std::memset(r->outlier, 0, n);
            }
            return CCM_OK;
        }
        const size_t m = (size_t)nl;
        size_t off = 0;
        const size_t o_status = seg(off, 16), o_out = seg(off, (size_t)n * 4), o_flag = seg(off, (size_t)n);
        const size_t o_lout = seg(off, p->last_outlier ? m : 0);
        const size_t o_head = seg(off, 16), pass_end = o_head + 16;
        const size_t o_pose = seg(off, 56), o_intr = seg(off, 32), o_is2 = seg(off, CCM_MAX_LEVELS * 4), o_scale = seg(off, CCM_MAX_LEVELS * 4);
        const size_t up_end = off;
        const size_t o_ninl = seg(off, 16), o_outl = seg(off, (size_t)n), o_ids = seg(off, (size_t)n * 4);
        const size_t res_end = o_ids + (size_t)n * 4;
        const size_t o_u = seg(off, m * 4), o_v = seg(off, m * 4), o_act = seg(off, m);
        const size_t tap_end = o_act + m;
        Staging& G = S.stage;
        if ((rc = G.reserve(c, off))) return rc;
        size_t w = 0;                                                          // device-only work area
        const size_t w_qr = seg(w, m * 4), w_minl = seg(w, m * 4), w_maxl = seg(w, m * 4), w_qflag = seg(w, m), w_qdesc = seg(w, m * 32);
        CCM_RESERVE(c, S.tmm, w + 64);
        uint8_t* wk = S.tmm.as<uint8_t>();

        G.put(o_lout, p->last_outlier, m);
        std::memset(G.host<uint8_t>(o_head), 0, up_end - o_head);
        if (pose) { G.put(o_pose, r->pose7, 56); G.put(o_intr, p->intr, 32); G.put(o_is2, p->inv_level_sigma2, (size_t)p->n_levels * 4); }
        G.put(o_scale, p->scale_factors, (size_t)p->n_levels * 4);
        if ((rc = G.upload(c, o_lout, up_end))) return rc;                     // 5 segments of 64 bytes, and last_outlier when given

        int* d_head = G.dev<int>(o_head); int* d_out = G.dev<int>(o_out); uint8_t* d_flag = G.dev<uint8_t>(o_flag);
        TmmArgs A{};
        A.n_last = nl; A.last_id = last->mp_id; A.last_outlier = p->last_outlier ? G.dev<uint8_t>(o_lout) : nullptr;
        std::memcpy(A.Tcw, p->Tcw, sizeof A.Tcw);
        A.fx = p->fx; A.fy = p->fy; A.cx = p->cx; A.cy = p->cy; A.min_x = p->min_x; A.max_x = p->max_x; A.min_y = p->min_y; A.max_y = p->max_y;
        A.qx = G.dev<float>(o_u); A.qy = G.dev<float>(o_v); A.act = G.dev<uint8_t>(o_act); A.qflag = wk + w_qflag; A.qdesc = wk + w_qdesc; A.head = d_head;
        tmm_launch_project(st, A, t->T);
        CCM_HIP(c, hipGetLastError());

        std::vector<uint8_t> occ(n);
        int nm = 0, passes = 0;
        for (int pass = 0; pass < 2; pass++) {
            const float th = pass == 0 ? p->th : 2.0f * p->th;
            tmm_launch_clear(st, n, nl, d_head, cur->mp_id, d_out, d_flag, A.act);
            frame_launch_prep_last(st, nl, A.act, last->oct, G.dev<float>(o_scale), th, (float*)(wk + w_qr), (int*)(wk + w_minl), (int*)(wk + w_maxl));
            CCM_HIP(c, hipGetLastError());
            WinDevCall D{ 2, nl, A.qx, A.qy, (const float*)(wk + w_qr), (const int*)(wk + w_minl), (const int*)(wk + w_maxl), A.qdesc, A.act, A.qflag,
                          last->mp_id, last->angle, o_status, o_out, o_flag, pass_end, 0.f, p->orb_dist, p->check_ori ? 1 : 0,
                          nullptr, nullptr, nullptr, last, nullptr, false };
            nm = frame_window_dev(c, cur, D, occ.data(), r->match);
            if (nm < 0) return nm;
            passes = pass + 1;
            if (pass == 0) {                                                   // the projection's verdict came back with the first pass
                int bad = 0;
                if (D.host_accept) { if ((rc = frame_fetch(c, &bad, d_head, 4))) return rc; }
                else G.get(&bad, o_head, 4);
                if (bad) return ccm_fail(c, CCM_E_ARG, "%s: last holds a map-point id outside [0, %d) or of a slot that is not LIVE", fn, t->capacity);
            }
            if (!(nm < p->retry_below)) break;
        }
        r->n_matches = nm; r->passes = passes;

        const bool posed = pose && nm >= p->min_matches;
        if (posed && (rc = frame_pose_queue(c, cur, t->T.capacity, t->T.pos, t->T.flags, p->n_levels, PoseIo{ o_ninl, o_outl, o_pose, o_intr, o_is2, 0 })))
            return rc;
        tmm_launch_discard(st, n, cur->mp_id, posed ? G.dev<uint8_t>(o_outl) : nullptr, t->T, G.dev<int>(o_ids), d_head);
        CCM_HIP(c, hipGetLastError());
        if ((rc = G.download(c, o_head, taps ? tap_end : res_end)) || (rc = G.wait(c))) return rc;
        int head[2], ninl[2] = { 0, 0 };
        G.get(head, o_head, 8);
        if (posed) {
            G.get(ninl, o_ninl, 8);
            if (ninl[1]) return ccm_fail(c, CCM_E_DEVICE, "%s: the pose stage met an id or octave it cannot use", fn);   // checked on entry and by the projection
            G.get(r->pose7, o_pose, 56);
            G.get(r->outlier, o_outl, n);
        } else std::memset(r->outlier, 0, n);
        G.get(r->mp_id, o_ids, (size_t)n * 4);
        r->posed = posed ? 1 : 0; r->n_inliers = ninl[0]; r->n_matches_map = head[1];
        G.get(r->u, o_u, m * 4); G.get(r->v, o_v, m * 4); G.get(r->valid, o_act, m);    // the taps: all three or none
        return CCM_OK;
    });
}

}  // extern "C"
