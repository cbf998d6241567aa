// frame_window_host.cpp -- the windowed matchers through a frame handle (include/ccm_hot.h "frame handles"): the two
// ccm_frame_search_by_projection* entry points and frame_window_dev, which SearchLocalPoints and TrackWithMotionModel share.
// Staging: [ status | match | occupied ] down, [ match (as -1) | occupied | qx | qy | qr | minl | maxl | qdesc | act | qflag |
// (qid) | (qang) | (scale) ] up; the occupancy flags sit at the seam and travel both ways.
#include "frame_internal.h"

// The windowed matchers through a handle.  mode 0: SearchByProjection(Frame, map points); mode 2: SearchByProjection(Frame,
// Frame | KeyFrame).  Queries come with their radius / level window (qr != nullptr) or, for a `last` handle, get them on the device.
struct WinCall {
    int mode, nq;
    const float* qx; const float* qy; const float* qr; const int32_t* minl; const int32_t* maxl;
    const uint8_t* qdesc; const uint8_t* active; const uint8_t* qflag; const int32_t* qid;
    const ccm_frame* last; const float* scale; float th;      // device-side query set-up (qr == nullptr)
    const float* q_angle;                                     // mode 2, check_ori, no `last`: the last side's angles (host)
    float nnratio; int orb_dist, check_ori;
};

static int frame_window(ccm_ctx* c, ccm_frame* f, const WinCall& w, uint8_t* occupied, int32_t* match)
{
    Staging& G = frame_state(c)->stage;
    hipStream_t st = c->stream;
    const int n = f->n, nq = w.nq;
    const bool dev_prep = w.qr == nullptr;
    const bool need_qang = w.mode == 2 && w.check_ori && !w.last;
    size_t off = 0;
    const size_t o_status = seg(off, 16), o_out = seg(off, (size_t)n * 4), o_flag = seg(off, (size_t)n);
    const size_t res_end = o_flag + n;
    const size_t o_qx = seg(off, (size_t)nq * 4), o_qy = seg(off, (size_t)nq * 4), o_qr = seg(off, (size_t)nq * 4);
    const size_t o_minl = seg(off, (size_t)nq * 4), o_maxl = seg(off, (size_t)nq * 4), o_qdesc = seg(off, (size_t)nq * 32);
    const size_t o_act = seg(off, (size_t)nq), o_qflag = seg(off, (size_t)nq);
    const size_t o_qid = seg(off, w.qid ? (size_t)nq * 4 : 0), o_qang = seg(off, need_qang ? (size_t)nq * 4 : 0);
    const size_t o_scale = seg(off, dev_prep ? (size_t)w.last->n_levels * 4 : 0);
    const size_t end = off;
    int rc = G.reserve(c, end);
    if (rc) return rc;
    std::memset(G.host<int>(o_out), 0xFF, (size_t)n * 4);
    G.put(o_flag, occupied, n);
    G.put(o_qx, w.qx, (size_t)nq * 4); G.put(o_qy, w.qy, (size_t)nq * 4);
    if (!dev_prep) {
        G.put(o_qr, w.qr, (size_t)nq * 4); G.put(o_minl, w.minl, (size_t)nq * 4); G.put(o_maxl, w.maxl, (size_t)nq * 4);
    } else {
        G.put(o_scale, w.scale, (size_t)w.last->n_levels * 4);
    }
    G.put(o_qdesc, w.qdesc, (size_t)nq * 32);
    G.put(o_act, w.active, nq); G.put(o_qflag, w.qflag, nq);
    G.put(o_qid, w.qid, (size_t)nq * 4);
    if (need_qang) G.put(o_qang, w.q_angle, (size_t)nq * 4);
    if ((rc = G.upload(c, o_out, end))) return rc;

    float* d_qr = G.dev<float>(o_qr); int* d_minl = G.dev<int>(o_minl); int* d_maxl = G.dev<int>(o_maxl);
    const uint8_t* d_act = G.dev<uint8_t>(o_act);
    const int* d_qid = w.qid ? G.dev<int>(o_qid) : nullptr;
    if (dev_prep) {
        frame_launch_prep_last(st, nq, d_act, w.last->oct, G.dev<float>(o_scale), w.th, d_qr, d_minl, d_maxl);
        CCM_HIP(c, hipGetLastError());
    }
    WinDevCall D{ w.mode, nq, G.dev<float>(o_qx), G.dev<float>(o_qy), d_qr, d_minl, d_maxl, G.dev<uint8_t>(o_qdesc), d_act, G.dev<uint8_t>(o_qflag),
                  d_qid ? d_qid : (w.last ? w.last->mp_id : nullptr),
                  need_qang ? G.dev<float>(o_qang) : (w.last ? w.last->angle : nullptr),
                  o_status, o_out, o_flag, res_end, w.nnratio, w.orb_dist, w.check_ori, w.active, w.qflag, w.q_angle, w.last, nullptr, false };
    return frame_window_dev(c, f, D, occupied, match);
}

int frame_window_dev(ccm_ctx* c, ccm_frame* f, WinDevCall& w, uint8_t* occupied, int32_t* match)
{
    FrameState& S = *frame_state(c);
    Staging& G = S.stage;
    hipStream_t st = c->stream;
    const int n = f->n, nq = w.nq;
    const size_t o_status = w.o_status, o_out = w.o_out, o_flag = w.o_flag, res_end = w.res_end;
    int* d_status = G.dev<int>(o_status); int* d_out = G.dev<int>(o_out); uint8_t* d_flag = G.dev<uint8_t>(o_flag);
    const uint8_t* d_act = w.act; const uint8_t* d_qflag = w.qflag; const int* id_src = w.id_src;
    int rc;
    w.host_accept = false;
    const WinLists L{ frame_win_grid(f), nullptr, nullptr, nq, w.qx, w.qy, w.qr, w.minl, w.maxl, w.qdesc, &S.ci, &S.cd, &S.cn };

    if (!window_host_accept_forced() && match_window_greedy_lds(n, nq) <= kGreedyLdsMax) {
        CCM_RESERVE(c, S.ev, std::max<size_t>((size_t)nq * 4, 16));
        GreedyArgs A{ nq, n, 0, nullptr, nullptr, nullptr, d_act, nullptr, f->oct, d_qflag, d_flag, w.nnratio,
                      d_out, d_status, w.orb_dist, w.check_ori, w.qang, f->angle, S.ev.as<int>(), nullptr };
        auto tail = [&] {                                                      // the new ids into the handle (none from an overflowed attempt)
            frame_launch_scatter_ids(st, n, d_out, id_src, d_status, f->mp_id);
            if (w.ids_copy) frame_launch_scatter_ids(st, n, d_out, id_src, d_status, w.ids_copy);
        };
        auto fetch = [&](const int** s) -> int { *s = G.host<int>(o_status); const int e = G.download(c, 0, res_end); return e ? e : G.wait(c); };
        const int* status = nullptr;                                           // one workgroup sees an overflow before it writes: nothing to reset
        if ((rc = window_greedy_drive(c, L, A, w.mode, 1, n, [] { return CCM_OK; }, tail, fetch, &status))) return rc;
        G.get(match, o_out, (size_t)n * 4);
        G.get(occupied, o_flag, n);
        return status[0];
    }

    // host acceptance (CCM_WINDOW_HOST_ACCEPT=1, or a frame too large for the single workgroup's LDS): lists to the host, the loops
    // of match_window_host.cpp on the frame's octaves / angles fetched from the device, the new ids scattered on the device
    w.host_accept = true;
    std::vector<uint8_t> act_h, qflag_h;
    const uint8_t* h_act = w.h_act; const uint8_t* h_qflag = w.h_qflag;
    if (!h_act) {                                                              // queries made on the device: their flags come back too
        act_h.resize(nq); qflag_h.resize(nq);
        if ((rc = frame_fetch(c, act_h.data(), d_act, nq)) || (rc = frame_fetch(c, qflag_h.data(), d_qflag, nq)) ||
            (rc = frame_fetch(c, occupied, d_flag, n))) return rc;
        h_act = act_h.data(); h_qflag = qflag_h.data();
        for (int i = 0; i < n; i++) match[i] = -1;
    }
    WinHostLists H{ 64 };
    if ((rc = window_lists_host(c, L, H))) return rc;
    int nmatches;
    if (w.mode == 0) {
        std::vector<int32_t> oct(n);
        if ((rc = frame_fetch(c, oct.data(), f->oct, (size_t)n * 4))) return rc;
        nmatches = window_accept_projection_host(nq, h_act, H.ci.data(), H.cd.data(), H.cn.data(), H.cap, oct.data(), h_qflag, occupied, w.nnratio, match);
    } else {
        std::vector<float> cur_angle, last_angle;
        if (w.check_ori) {
            cur_angle.resize(n);
            if ((rc = frame_fetch(c, cur_angle.data(), f->angle, (size_t)n * 4))) return rc;
            if (w.last) { last_angle.resize(nq); if ((rc = frame_fetch(c, last_angle.data(), w.last->angle, (size_t)nq * 4))) return rc; }
        }
        nmatches = window_accept_frame_host(nq, h_act, H.ci.data(), H.cd.data(), H.cn.data(), H.cap, h_qflag, occupied, w.orb_dist, w.check_ori,
                                            w.last ? last_angle.data() : w.h_qang, cur_angle.data(), match);
    }
    G.put(o_out, match, (size_t)n * 4);                                      // the stream is idle: the staging area is free
    if ((rc = G.upload(c, o_out, o_out + (size_t)n * 4))) return rc;
    frame_launch_scatter_ids(st, n, d_out, id_src, nullptr, f->mp_id);
    CCM_HIP(c, hipGetLastError());
    return nmatches;
}

extern "C" {

// ORBmatcher::SearchByProjection(Frame&, const vector<mpptr>&, th), ORBmatcher.cpp:71-148, frame side from the handle
int ccm_frame_search_by_projection(ccm_ctx* c, ccm_frame* f, const float* scale_factors, int n_mp, const uint8_t* in_view,
                                   const int32_t* level, const float* view_cos, const float* proj_x, const float* proj_y,
                                   const uint8_t* mp_desc, const uint8_t* mp_has_obs, const int32_t* query_mp_id,
                                   uint8_t* occupied, float th, float nnratio, int32_t* match)
{
    RoctxRange roctx_("ccm_frame_search_by_projection");
    if (!c || !f) return CCM_E_ARG;
    int rc = frame_check(c, f);
    if (rc) return rc;
    if (n_mp < 0 || (f->n > 0 && (!match || !occupied)) ||
        (n_mp > 0 && (!scale_factors || !in_view || !level || !view_cos || !proj_x || !proj_y || !mp_desc || !mp_has_obs)))
        return ccm_fail(c, CCM_E_ARG, "bad SearchByProjection arguments");
    for (int i = 0; i < f->n; i++) match[i] = -1;
    if (n_mp == 0 || f->n == 0) return 0;
    return ccm_guard(c, "ccm_frame_search_by_projection", [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        const WinQueries q = window_queries_projection(n_mp, in_view, level, view_cos, scale_factors, th);
        WinCall w{ 0, n_mp, proj_x, proj_y, q.qr.data(), q.minl.data(), q.maxl.data(), mp_desc, in_view, mp_has_obs, query_mp_id,
                   nullptr, nullptr, 0.f, nullptr, nnratio, 0, 0 };
        return frame_window(c, f, w, occupied, match);
    });
}

// ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th), ORBmatcher.cpp:1350-1476, and the relocalisation
// overload (:1478-1605), current frame (and last frame) from handles
int ccm_frame_search_by_projection_frame(ccm_ctx* c, ccm_frame* cur, const ccm_frame* last, const float* scale_factors, int n_last,
                                         const uint8_t* valid, const float* u, const float* v, const int32_t* last_octave,
                                         const float* last_angle, const uint8_t* mp_desc, const uint8_t* mp_has_obs,
                                         const int32_t* query_mp_id, uint8_t* occupied, float th, int check_ori, int orb_dist,
                                         int32_t* match)
{
    RoctxRange roctx_("ccm_frame_search_by_projection_frame");
    if (!c || !cur) return CCM_E_ARG;
    int rc = frame_check(c, cur);
    if (rc || (last && (rc = frame_check(c, last)))) return rc;
    if (n_last < 0 || (last && n_last != last->n)) return ccm_fail(c, CCM_E_ARG, "n_last must be >= 0 and equal the last frame's N");
    if (check_ori && (!cur->has_angle || (last && !last->has_angle)))
        return ccm_fail(c, CCM_E_ARG, "orientation check against a frame created without angles");
    if ((cur->n > 0 && (!match || !occupied)) ||
        (n_last > 0 && (!scale_factors || !valid || !u || !v || !mp_desc || !mp_has_obs || (!last && (!last_octave || (check_ori && !last_angle))))))
        return ccm_fail(c, CCM_E_ARG, "bad SearchByProjection(frame, frame) arguments");
    for (int i = 0; i < cur->n; i++) match[i] = -1;
    if (n_last == 0 || cur->n == 0) return 0;
    return ccm_guard(c, "ccm_frame_search_by_projection_frame", [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        WinQueries q;                                                          // a `last` handle: set up on the device
        if (!last) q = window_queries_frame(n_last, valid, last_octave, scale_factors, th);
        WinCall w{ 2, n_last, u, v, last ? nullptr : q.qr.data(), last ? nullptr : q.minl.data(), last ? nullptr : q.maxl.data(), mp_desc, valid,
                   mp_has_obs, query_mp_id, last, scale_factors, th, last_angle, 0.f, orb_dist, check_ori ? 1 : 0 };
        return frame_window(c, cur, w, occupied, match);
    });
}

}  // extern "C"
