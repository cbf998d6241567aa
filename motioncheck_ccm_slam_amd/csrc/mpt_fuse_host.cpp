// mpt_fuse_host.cpp -- ORBmatcher::Fuse on the map-point table and keyframe handles (include/ccm_hot.h "map-point table"), up to the
// selection, for every (keyframe, point) pair of a call.  It stages through the frame handles' block (the layout: at the entry point)
// and keeps the query list and the selections in device memory.
#include "mpt_internal.h"

// what a keyframe costs in the staging copy of ccm_fuse_select_table_frames (tools/bench_fuse_table.py counts the upload with these)
static_assert(sizeof(FuseView) == 112 && sizeof(WinGrid) == 80, "per-keyframe upload of ccm_fuse_select_table_frames");

extern "C" {

// ORBmatcher::Fuse, both overloads (src/ORBmatcher.cpp:854-1000, :1002-1122), up to the selection, for every (keyframe, point) pair.
// Staging: [ count | best_idx | best_dist | gate | u | v | level ] down, [ views | grids | slot | skip | inv_level_sigma2 ] up; the
// taps take room only when asked for.  The query list and the selections stay in device memory (FrameState::fuse).
int ccm_fuse_select_table_frames(ccm_ctx* c, ccm_map_table* t, const ccm_fuse_table_problem* p, ccm_fuse_table_result* r)
{
    RoctxRange roctx_("ccm_fuse_select_table_frames");
    if (!c || !t || !p || !r) return CCM_E_ARG;
    const char* fn = "ccm_fuse_select_table_frames";
    int rc = check_table(c, t);
    if (rc) return rc;
    if (p->n_kf < 0 || p->n_points < 0) return ccm_fail(c, CCM_E_ARG, "%s: n_kf = %d, n_points = %d", fn, p->n_kf, p->n_points);
    if (p->n_kf == 0 || p->n_points == 0) { r->n_searched = 0; return CCM_OK; }
    if (!p->views || !p->slot || !p->scale_factors || !r->best_idx || (p->chi2_check && !p->inv_level_sigma2))
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !p->views ? "views" : !p->slot ? "slot" : !p->scale_factors ? "scale_factors" :
                        !r->best_idx ? "best_idx" : "inv_level_sigma2 with chi2_check");
    if (p->n_levels < 1 || p->n_levels > CCM_MAX_LEVELS) return ccm_fail(c, CCM_E_ARG, "%s: n_levels = %d outside 1..%d", fn, p->n_levels, CCM_MAX_LEVELS);
    if ((r->u || r->v || r->level) && !(r->u && r->v && r->level)) return ccm_fail(c, CCM_E_ARG, "%s: the taps u, v and level come together", fn);
    if (p->n_kf > 65535 || (size_t)p->n_kf * (size_t)p->n_points > ((size_t)1 << 24))
        return ccm_fail(c, CCM_E_CAPACITY, "%s: %d keyframes x %d points; at most 65535 keyframes and 2^24 pairs a call", fn, p->n_kf, p->n_points);
    return table_call(c, t, false, fn, [&]() -> int {                          // writes the handle's own where[] only
        const int n_kf = p->n_kf, n_pt = p->n_points;
        int max_n = 0;
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* f = p->views[k].kf;
            if (!f) return ccm_fail(c, CCM_E_ARG, "%s: null views[%d].kf", fn, k);
            if ((rc = frame_named_check(c, f, CCM_E_STATE, fn, "views[%d].kf", k))) return rc;
            max_n = std::max(max_n, f->n);
        }
        bool dup = false;
        if ((rc = mark_slots(c, t, n_pt, p->slot, &dup))) return rc;
        if (dup) return ccm_fail(c, CCM_E_ARG, "%s: a slot is listed twice", fn);

        CCM_HIP(c, hipSetDevice(c->device));
        FrameState& S = *frame_state(c);
        Staging& G = S.stage;
        hipStream_t st = c->stream;
        const size_t m = (size_t)n_kf * (size_t)n_pt;
        const bool taps = r->u != nullptr;
        size_t off = 0;
        const size_t o_cnt = seg(off, 16), o_bi = seg(off, m * 4), o_bd = seg(off, r->best_dist ? m * 4 : 0), o_gate = seg(off, r->gate ? m : 0);
        const size_t o_u = seg(off, taps ? m * 4 : 0), o_v = seg(off, taps ? m * 4 : 0), o_lvl = seg(off, taps ? m * 4 : 0);
        const size_t res_end = off;
        const size_t o_view = seg(off, (size_t)n_kf * sizeof(FuseView)), o_grid = seg(off, (size_t)n_kf * sizeof(WinGrid));
        const size_t o_slot = seg(off, (size_t)n_pt * 4), o_skip = seg(off, p->skip ? (size_t)n_pt : 0);
        const size_t o_is2 = seg(off, p->chi2_check ? CCM_MAX_LEVELS * 4 : 0);
        const size_t end = off;
        if ((rc = G.reserve(c, end))) return rc;
        size_t w = 0;                                                          // device-only work area
        const size_t w_held = seg(w, m), w_qx = seg(w, m * 4), w_qy = seg(w, m * 4), w_qr = seg(w, m * 4), w_minl = seg(w, m * 4), w_maxl = seg(w, m * 4);
        const size_t w_qkf = seg(w, m * 4), w_qpair = seg(w, m * 4), w_qdesc = seg(w, m * 32), w_si = seg(w, m * 4), w_sd = seg(w, m * 4);
        CCM_RESERVE(c, S.fuse, w + 64);
        unsigned stamp = 0;
        if ((rc = next_where_stamp(c, t, st, &stamp))) return rc;

        FuseView* hv = G.host<FuseView>(o_view); WinGrid* hg = G.host<WinGrid>(o_grid);
        for (int k = 0; k < n_kf; k++) {
            fuse_view_fill(hv[k], p->views[k]);
            hg[k] = frame_win_grid(p->views[k].kf);
        }
        G.put(o_slot, p->slot, (size_t)n_pt * 4);
        G.put(o_skip, p->skip, (size_t)n_pt);
        if (p->chi2_check) fill_levels(G.host<float>(o_is2), p->inv_level_sigma2, p->n_levels);
        if ((rc = G.upload(c, o_view, end))) return rc;
        uint8_t* wk = S.fuse.as<uint8_t>();
        FuseArgs A{};
        A.n_kf = n_kf; A.n_points = n_pt;
        A.views = G.dev<FuseView>(o_view); A.slot = G.dev<int>(o_slot); A.skip = p->skip ? G.dev<uint8_t>(o_skip) : nullptr;
        A.where = t->where.as<unsigned long long>(); A.stamp = stamp; A.held = wk + w_held;
        A.log_scale = p->log_scale_factor; A.n_levels = p->n_levels; A.th = p->th;
        fill_levels(A.scale, p->scale_factors, p->n_levels);
        A.best_idx = G.dev<int>(o_bi); A.best_dist = r->best_dist ? G.dev<int>(o_bd) : nullptr; A.gate = r->gate ? G.dev<uint8_t>(o_gate) : nullptr;
        A.u = taps ? G.dev<float>(o_u) : nullptr; A.v = taps ? G.dev<float>(o_v) : nullptr; A.level = taps ? G.dev<int>(o_lvl) : nullptr;
        A.cnt = G.dev<int>(o_cnt); A.qx = (float*)(wk + w_qx); A.qy = (float*)(wk + w_qy); A.qr = (float*)(wk + w_qr);
        A.minl = (int*)(wk + w_minl); A.maxl = (int*)(wk + w_maxl); A.qkf = (int*)(wk + w_qkf); A.qpair = (int*)(wk + w_qpair); A.qdesc = wk + w_qdesc;
        CCM_HIP(c, hipMemsetAsync(A.cnt, 0, 16, st));
        CCM_HIP(c, hipMemsetAsync(A.held, 0, m, st));
        fuse_launch_project(st, A, t->T, max_n);
        CCM_HIP(c, hipGetLastError());
        if ((rc = G.download(c, 0, 16)) || (rc = G.wait(c))) return rc;        // the number of queries: the first synchronisation
        int nq = 0;
        G.get(&nq, o_cnt, 4);
        if (nq < 0 || (size_t)nq > m) return ccm_fail(c, CCM_E_DEVICE, "%s: %d queries of %zu pairs", fn, nq, m);
        if (nq > 0) {
            match_launch_window_select_batch(st, G.dev<WinGrid>(o_grid), A.qkf, nq, A.qx, A.qy, A.qr, A.minl, A.maxl, A.qdesc,
                                             p->chi2_check ? G.dev<float>(o_is2) : nullptr, p->accept_th, (int*)(wk + w_si), (int*)(wk + w_sd));
            fuse_launch_scatter(st, nq, (int)m, A.qpair, (const int*)(wk + w_si), (const int*)(wk + w_sd), A.best_idx, A.best_dist);
            CCM_HIP(c, hipGetLastError());
        }
        if ((rc = G.download(c, 0, res_end)) || (rc = G.wait(c))) return rc;   // the second
        G.get(r->best_idx, o_bi, m * 4); G.get(r->best_dist, o_bd, m * 4); G.get(r->gate, o_gate, m);
        G.get(r->u, o_u, m * 4); G.get(r->v, o_v, m * 4); G.get(r->level, o_lvl, m * 4);    // the taps: all three or none
        r->n_searched = nq;
        return CCM_OK;
    });
}

}  // extern "C"
