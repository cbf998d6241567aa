// mpt_sim3_host.cpp -- ComputeSim3's two matchers on keyframe handles and the map-point table (include/ccm_hot.h "ComputeSim3 on
// keyframe handles and the table"): ORBmatcher::SearchBySim3 for a batch of candidate pairs, and SearchByProjection(pKF, Scw, ...) for a
// batch of views of one slot list.  Both stage through the frame handles' block (the layouts: at the entry points) and keep the
// queries, the candidate lists and the selections in device memory (FrameState::fuse, ci / cd / cn).
#include "mpt_internal.h"

// what a pair or a view costs in the staging copies (tools/bench_compute_sim3_table.py counts the uploads with these)
static_assert(sizeof(Sim3View) == 168 && sizeof(Sim3Pair) == 16 && sizeof(WinGrid) == 80, "per-pair upload of ccm_search_by_sim3_table_frames");
static_assert(sizeof(FuseView) == 112 && sizeof(GreedyKf) == 16, "per-view upload of ccm_search_by_projection_table_frames");

// What ccm_search_by_sim3_table_frames refuses before it takes the lock; n_pairs == 0 passes
int sim3_search_check(ccm_ctx* c, const ccm_map_table* t, const ccm_sim3_search_problem* p, const ccm_sim3_search_result* r, const char* fn)
{
    int rc = check_table(c, t);
    if (rc) return rc;
    if (p->n_pairs < 0) return ccm_fail(c, CCM_E_ARG, "%s: n_pairs = %d", fn, p->n_pairs);
    if (p->n_pairs == 0) return CCM_OK;
    if (!p->pairs || !p->scale_factors1 || !p->scale_factors2 || !r->n_found)
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !p->pairs ? "pairs" : !r->n_found ? "n_found" : "scale_factors1 / scale_factors2");
    if (p->n_levels1 < 1 || p->n_levels1 > CCM_MAX_LEVELS || p->n_levels2 < 1 || p->n_levels2 > CCM_MAX_LEVELS)
        return ccm_fail(c, CCM_E_ARG, "%s: n_levels = %d, %d outside 1..%d", fn, p->n_levels1, p->n_levels2, CCM_MAX_LEVELS);
    if (((r->u1 || r->v1 || r->level1) && !(r->u1 && r->v1 && r->level1)) || ((r->u2 || r->v2 || r->level2) && !(r->u2 && r->v2 && r->level2)))
        return ccm_fail(c, CCM_E_ARG, "%s: the taps u, v and level of a direction come together", fn);
    if (p->n_pairs > 32767) return ccm_fail(c, CCM_E_CAPACITY, "%s: %d pairs; at most 32767 a call", fn, p->n_pairs);
    return CCM_OK;
}

// The pipeline of ccm_search_by_sim3_table_frames, whose arguments the entry point has checked, under the table's lock
int sim3_search_run(ccm_ctx* c, ccm_map_table* t, const ccm_sim3_search_problem* p, ccm_sim3_search_result* r, const char* fn, Sim3Chain* chain)
{
    int rc;
    const int n_pairs = p->n_pairs, n_views = 2 * n_pairs;
    std::vector<Sim3Pair> pr(n_pairs);
    size_t sum1 = 0, sum2 = 0;
    int max_n = 0, max_n1 = 0;
    for (int k = 0; k < n_pairs; k++) {
        const ccm_sim3_search_pair& P = p->pairs[k];
        if (!P.kf1 || !P.kf2) return ccm_fail(c, CCM_E_ARG, "%s: null pairs[%d].%s", fn, k, !P.kf1 ? "kf1" : "kf2");
        if ((rc = frame_named_check(c, P.kf1, CCM_E_STATE, fn, "pairs[%d].kf1", k)) || (rc = frame_named_check(c, P.kf2, CCM_E_STATE, fn, "pairs[%d].kf2", k)))
            return rc;
        if (P.kf1->n > 0 && (!P.matched12 || !P.matched_idx2)) return ccm_fail(c, CCM_E_ARG, "%s: null pairs[%d].matched12 / matched_idx2", fn, k);
        pr[k] = Sim3Pair{ P.kf1->n, P.kf2->n, (int)sum1, (int)sum2 };
        sum1 += (size_t)P.kf1->n; sum2 += (size_t)P.kf2->n;
        max_n = std::max(max_n, std::max(P.kf1->n, P.kf2->n)); max_n1 = std::max(max_n1, P.kf1->n);
        if (sum1 + sum2 > ((size_t)1 << 24)) return ccm_fail(c, CCM_E_CAPACITY, "%s: more than 2^24 features in one call", fn);
    }
    if (sum1 > 0 && !r->match12) return ccm_fail(c, CCM_E_ARG, "%s: null match12", fn);
    const size_t E = sum1 + sum2;
    if (E == 0 || max_n1 == 0) {                                           // no feature on side 1: nothing can match
        for (int k = 0; k < n_pairs; k++) r->n_found[k] = 0;
        if (E == 0) { if (chain) chain->none(); return 0; }
    }
    if (chain) chain->size(n_pairs, sum1);

    CCM_HIP(c, hipSetDevice(c->device));
    FrameState& S = *frame_state(c);
    Staging& G = S.stage;
    hipStream_t st = c->stream;
    const bool tap_sel = r->sel1 || r->sel2, tap_gate = r->gate1 || r->gate2, taps = r->u1 || r->u2;
    size_t off = 0;
    const size_t o_cnt = seg(off, 16), o_m12 = seg(off, sum1 * 4), o_sel = seg(off, tap_sel ? E * 4 : 0), o_gate = seg(off, tap_gate ? E : 0);
    const size_t o_u = seg(off, taps ? E * 4 : 0), o_v = seg(off, taps ? E * 4 : 0), o_lvl = seg(off, taps ? E * 4 : 0);
    const size_t o_chain = seg(off, chain ? chain->res_bytes : 0);
    const size_t res_end = off;
    const size_t o_view = seg(off, (size_t)n_views * sizeof(Sim3View)), o_grid = seg(off, (size_t)n_views * sizeof(WinGrid));
    const size_t o_pair = seg(off, (size_t)n_pairs * sizeof(Sim3Pair)), o_mi = seg(off, sum1 * 4), o_mx = seg(off, sum1 * 4);
    const size_t o_chin = seg(off, chain ? chain->in_bytes : 0);
    const size_t end = off;
    if ((rc = G.reserve(c, end))) return rc;
    size_t w = 0;                                                          // device-only work area
    const size_t w_am2 = seg(w, sum2), w_sel = seg(w, tap_sel ? 0 : E * 4), w_qx = seg(w, E * 4), w_qy = seg(w, E * 4), w_qr = seg(w, E * 4);
    const size_t w_minl = seg(w, E * 4), w_maxl = seg(w, E * 4), w_qview = seg(w, E * 4), w_qent = seg(w, E * 4), w_qdesc = seg(w, E * 32);
    const size_t w_si = seg(w, E * 4), w_sd = seg(w, E * 4), w_chain = seg(w, chain ? chain->work_bytes : 0);
    CCM_RESERVE(c, S.fuse, w + 64);
    uint8_t* wk = S.fuse.as<uint8_t>();

    Sim3View* hv = G.host<Sim3View>(o_view); WinGrid* hg = G.host<WinGrid>(o_grid);
    const int* d_mi = G.dev<int>(o_mi);
    for (int k = 0; k < n_pairs; k++) {
        const ccm_sim3_search_pair& P = p->pairs[k];
        for (int d = 0; d < 2; d++) {
            const ccm_frame* src = d ? P.kf2 : P.kf1; const ccm_frame* dst = d ? P.kf1 : P.kf2;
            const float* bounds = d ? P.bounds1 : P.bounds2;
            Sim3View& D = hv[2 * k + d];
            std::memcpy(D.Tsw, d ? P.T2w : P.T1w, sizeof D.Tsw); std::memcpy(D.Sts, d ? P.S12 : P.S21, sizeof D.Sts);
            D.fx = P.fx; D.fy = P.fy; D.cx = P.cx; D.cy = P.cy;
            D.min_x = bounds[0]; D.max_x = bounds[1]; D.min_y = bounds[2]; D.max_y = bounds[3];
            D.n = src->n; D.n_target = dst->n; D.e0 = d ? (int)sum1 + pr[k].first2 : pr[k].first1; D.side_t = d ? 0 : 1;
            D.mp_id = src->mp_id;
            D.mark_i = d ? nullptr : d_mi + pr[k].first1;
            D.mark_b = d ? wk + w_am2 + pr[k].first2 : nullptr;
            hg[2 * k + d] = frame_win_grid(dst);
        }
        G.put(o_mi + (size_t)pr[k].first1 * 4, P.matched12, (size_t)pr[k].n1 * 4);
        G.put(o_mx + (size_t)pr[k].first1 * 4, P.matched_idx2, (size_t)pr[k].n1 * 4);
    }
    std::memcpy(G.host<Sim3Pair>(o_pair), pr.data(), (size_t)n_pairs * sizeof(Sim3Pair));
    if (chain) chain->fill(G, o_chin);
    if ((rc = G.upload(c, o_view, end))) return rc;

    Sim3Args A{};
    A.n_views = n_views; A.n_entries = (int)E; A.views = G.dev<Sim3View>(o_view);
    A.log_scale[0] = p->log_scale_factor1; A.log_scale[1] = p->log_scale_factor2; A.n_levels[0] = p->n_levels1; A.n_levels[1] = p->n_levels2;
    fill_levels(A.scale[0], p->scale_factors1, p->n_levels1); fill_levels(A.scale[1], p->scale_factors2, p->n_levels2);
    A.th = p->th;
    A.sel = tap_sel ? G.dev<int>(o_sel) : (int*)(wk + w_sel);
    A.gate = tap_gate ? G.dev<uint8_t>(o_gate) : nullptr;
    A.u = taps ? G.dev<float>(o_u) : nullptr; A.v = taps ? G.dev<float>(o_v) : nullptr; A.level = taps ? G.dev<int>(o_lvl) : nullptr;
    A.cnt = G.dev<int>(o_cnt); A.qx = (float*)(wk + w_qx); A.qy = (float*)(wk + w_qy); A.qr = (float*)(wk + w_qr);
    A.minl = (int*)(wk + w_minl); A.maxl = (int*)(wk + w_maxl); A.qview = (int*)(wk + w_qview); A.qent = (int*)(wk + w_qent); A.qdesc = wk + w_qdesc;
    const Sim3Pair* d_pair = G.dev<Sim3Pair>(o_pair);
    CCM_HIP(c, hipMemsetAsync(A.cnt, 0, 16, st));
    if (sum2) CCM_HIP(c, hipMemsetAsync(wk + w_am2, 0, sum2, st));
    sim3_launch_marks(st, n_pairs, max_n1, d_pair, d_mi, G.dev<int>(o_mx), wk + w_am2);
    sim3_launch_project(st, A, t->T, max_n);
    CCM_HIP(c, hipGetLastError());
    if ((rc = G.download(c, 0, 16)) || (rc = G.wait(c))) return rc;        // the number of queries: the first synchronisation
    int nq = 0;
    G.get(&nq, o_cnt, 4);
    if (nq < 0 || (size_t)nq > E) return ccm_fail(c, CCM_E_DEVICE, "%s: %d queries of %zu features", fn, nq, E);
    if (nq > 0) {
        match_launch_window_select_batch(st, G.dev<WinGrid>(o_grid), A.qview, nq, A.qx, A.qy, A.qr, A.minl, A.maxl, A.qdesc, nullptr, 100,   // TH_HIGH
                                         (int*)(wk + w_si), (int*)(wk + w_sd));
        fuse_launch_scatter(st, nq, (int)E, A.qent, (const int*)(wk + w_si), (const int*)(wk + w_sd), A.sel, nullptr);
    }
    sim3_launch_agree(st, n_pairs, max_n1, d_pair, A.sel, (int)sum1, G.dev<int>(o_m12));
    CCM_HIP(c, hipGetLastError());
    if (chain && (rc = chain->queue(c, t->T, G, o_chain, o_chin, wk + w_chain, max_n1, d_pair, d_mi, G.dev<int>(o_mx), G.dev<int>(o_m12)))) return rc;
    if ((rc = G.download(c, 0, res_end)) || (rc = G.wait(c))) return rc;   // the second
    if (chain && (rc = chain->deliver(c, G, o_chain, o_chin))) return rc;
    G.get(r->match12, o_m12, sum1 * 4);
    G.get(r->sel1, o_sel, sum1 * 4); G.get(r->sel2, o_sel + sum1 * 4, sum2 * 4);
    G.get(r->gate1, o_gate, sum1); G.get(r->gate2, o_gate + sum1, sum2);
    G.get(r->u1, o_u, sum1 * 4); G.get(r->v1, o_v, sum1 * 4); G.get(r->level1, o_lvl, sum1 * 4);
    G.get(r->u2, o_u + sum1 * 4, sum2 * 4); G.get(r->v2, o_v + sum1 * 4, sum2 * 4); G.get(r->level2, o_lvl + sum1 * 4, sum2 * 4);
    int total = 0;
    const int* m12 = G.host<int>(o_m12);
    for (int k = 0; k < n_pairs; k++) {
        int found = 0;
        for (int i = 0; i < pr[k].n1; i++) found += m12[pr[k].first1 + i] >= 0;
        r->n_found[k] = found; total += found;
    }
    return total;
}

extern "C" {

// ORBmatcher::SearchBySim3 (src/ORBmatcher.cpp:1124-1348) for n_pairs candidate pairs.  Entries: the features of every side-1 handle,
// then of every side-2 handle.  Staging: [ count | match12 | (sel) | (gate) | (u | v | level) ] down, [ views | grids | pairs |
// matched12 | matched_idx2 ] up; the taps take room only when asked for.
int ccm_search_by_sim3_table_frames(ccm_ctx* c, ccm_map_table* t, const ccm_sim3_search_problem* p, ccm_sim3_search_result* r)
{
    RoctxRange roctx_("ccm_search_by_sim3_table_frames");
    if (!c || !t || !p || !r) return CCM_E_ARG;
    const char* fn = "ccm_search_by_sim3_table_frames";
    const int rc = sim3_search_check(c, t, p, r, fn);
    if (rc || p->n_pairs == 0) return rc;
    return table_call(c, t, false, fn, [&]() -> int { return sim3_search_run(c, t, p, r, fn, nullptr); });
}

// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cpp:308-446) for n_kf views of one slot list.
// Staging: [ status | best_idx | observed | matched_slot | (best_dist) | (gate) | (u | v | level) ] down, [ views | grids | query
// ranges | feature offsets | slot | matched_slot ] up.
int ccm_search_by_projection_table_frames(ccm_ctx* c, ccm_map_table* t, const ccm_loop_projection_problem* p, ccm_loop_projection_result* r)
{
    RoctxRange roctx_("ccm_search_by_projection_table_frames");
    if (!c || !t || !p || !r) return CCM_E_ARG;
    const char* fn = "ccm_search_by_projection_table_frames";
    int rc = check_table(c, t);
    if (rc) return rc;
    if (p->n_kf < 0 || p->n_points < 0) return ccm_fail(c, CCM_E_ARG, "%s: n_kf = %d, n_points = %d", fn, p->n_kf, p->n_points);
    if (p->n_kf == 0) return 0;
    if (!p->views || !r->n_matches) return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !p->views ? "views" : "n_matches");
    if (p->n_points > 0 && (!p->slot || !p->scale_factors || !r->best_idx || !r->observed))
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !p->slot ? "slot" : !p->scale_factors ? "scale_factors" : !r->best_idx ? "best_idx" : "observed");
    if (p->n_points > 0 && (p->n_levels < 1 || p->n_levels > CCM_MAX_LEVELS))
        return ccm_fail(c, CCM_E_ARG, "%s: n_levels = %d outside 1..%d", fn, p->n_levels, CCM_MAX_LEVELS);
    if ((r->u || r->v || r->level) && !(r->u && r->v && r->level)) return ccm_fail(c, CCM_E_ARG, "%s: the taps u, v and level come together", fn);
    if (p->n_kf > 65535 || (size_t)p->n_kf * (size_t)p->n_points > ((size_t)1 << 24))
        return ccm_fail(c, CCM_E_CAPACITY, "%s: %d views x %d points; at most 65535 views and 2^24 pairs a call", fn, p->n_kf, p->n_points);
    return table_call(c, t, false, fn, [&]() -> int {                          // writes the handle's own where[] only
        const int n_kf = p->n_kf, n_pt = p->n_points;
        std::vector<int> ff(n_kf + 1, 0);
        int max_n = 0;
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* f = p->views[k].view.kf;
            if (!f) return ccm_fail(c, CCM_E_ARG, "%s: null views[%d].kf", fn, k);
            if ((rc = frame_named_check(c, f, CCM_E_STATE, fn, "views[%d].kf", k))) return rc;
            if (f->n > 0 && !p->views[k].matched_slot) return ccm_fail(c, CCM_E_ARG, "%s: null views[%d].matched_slot", fn, k);
            if ((size_t)ff[k] + (size_t)f->n > ((size_t)1 << 30)) return ccm_fail(c, CCM_E_CAPACITY, "%s: too many features", fn);
            ff[k + 1] = ff[k] + f->n;
            max_n = std::max(max_n, f->n);
        }
        const size_t NF = (size_t)ff[n_kf];
        if (NF > 0 && !r->matched_slot) return ccm_fail(c, CCM_E_ARG, "%s: null matched_slot of the result", fn);
        bool dup = false;
        if ((rc = mark_slots(c, t, n_pt, p->slot, &dup))) return rc;
        if (dup) return ccm_fail(c, CCM_E_ARG, "%s: a slot is listed twice", fn);
        if (n_pt == 0) {                                                       // nothing to project: vpMatched passes through
            for (int k = 0; k < n_kf; k++) {
                r->n_matches[k] = 0;
                if (ff[k + 1] > ff[k]) std::memcpy(r->matched_slot + ff[k], p->views[k].matched_slot, (size_t)(ff[k + 1] - ff[k]) * 4);
            }
            return 0;
        }

        CCM_HIP(c, hipSetDevice(c->device));
        FrameState& S = *frame_state(c);
        Staging& G = S.stage;
        hipStream_t st = c->stream;
        const size_t m = (size_t)n_kf * (size_t)n_pt;
        const bool taps = r->u != nullptr;
        size_t off = 0;
        const size_t o_status = seg(off, (size_t)n_kf * 12), o_bi = seg(off, m * 4), o_obs = seg(off, m), o_ms = seg(off, NF * 4);
        const size_t o_bd = seg(off, r->best_dist ? m * 4 : 0), o_gate = seg(off, r->gate ? m : 0);
        const size_t o_u = seg(off, taps ? m * 4 : 0), o_v = seg(off, taps ? m * 4 : 0), o_lvl = seg(off, taps ? m * 4 : 0);
        const size_t res_end = off;
        const size_t o_view = seg(off, (size_t)n_kf * sizeof(FuseView)), o_grid = seg(off, (size_t)n_kf * sizeof(WinGrid));
        const size_t o_gk = seg(off, (size_t)n_kf * sizeof(GreedyKf)), o_ff = seg(off, (size_t)n_kf * 4);
        const size_t o_slot = seg(off, (size_t)n_pt * 4), o_msin = seg(off, NF * 4);
        const size_t end = off;
        if ((rc = G.reserve(c, end))) return rc;
        size_t w = 0;                                                          // device-only work area
        const size_t w_found = seg(w, m), w_qx = seg(w, m * 4), w_qy = seg(w, m * 4), w_qr = seg(w, m * 4), w_none = seg(w, m * 4), w_qkf = seg(w, m * 4);
        const size_t w_qlvl = seg(w, m * 4), w_act = seg(w, m), w_qdesc = seg(w, m * 32), w_flag = seg(w, NF), w_oct = seg(w, NF * 4);
        CCM_RESERVE(c, S.fuse, w + 64);
        uint8_t* wk = S.fuse.as<uint8_t>();
        unsigned stamp = 0;
        if ((rc = next_where_stamp(c, t, st, &stamp))) return rc;

        FuseView* hv = G.host<FuseView>(o_view); WinGrid* hg = G.host<WinGrid>(o_grid); GreedyKf* gk = G.host<GreedyKf>(o_gk);
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* f = p->views[k].view.kf;
            fuse_view_fill(hv[k], p->views[k].view);
            hg[k] = frame_win_grid(f);
            gk[k] = GreedyKf{ k * n_pt, n_pt, ff[k], f->n };
            G.put(o_msin + (size_t)ff[k] * 4, p->views[k].matched_slot, (size_t)f->n * 4);
        }
        G.put(o_ff, ff.data(), (size_t)n_kf * 4);
        G.put(o_slot, p->slot, (size_t)n_pt * 4);
        if ((rc = G.upload(c, o_view, end))) return rc;

        const WinGrid* d_grid = G.dev<WinGrid>(o_grid); const int* d_ff = G.dev<int>(o_ff); const int* d_slot = G.dev<int>(o_slot);
        uint8_t* d_held = G.dev<uint8_t>(o_obs); uint8_t* d_found = wk + w_found; uint8_t* d_flag = wk + w_flag; int* d_oct = (int*)(wk + w_oct);
        int* d_ms = G.dev<int>(o_ms); int* d_out = G.dev<int>(o_bi); int* d_status = G.dev<int>(o_status);
        FuseArgs M{};                                                          // the membership lookups of Fuse: where[] and `observed`
        M.n_kf = n_kf; M.n_points = n_pt; M.views = G.dev<FuseView>(o_view); M.slot = d_slot;
        M.where = t->where.as<unsigned long long>(); M.stamp = stamp; M.held = d_held;
        CCM_HIP(c, hipMemsetAsync(d_held, 0, m, st));
        CCM_HIP(c, hipMemsetAsync(d_found, 0, m, st));
        CCM_HIP(c, hipMemsetAsync(d_status, 0, (size_t)n_kf * 12, st));
        fuse_launch_membership(st, M, t->T, max_n);
        auto marks = [&]() {
            loop_launch_marks(st, n_kf, n_pt, max_n, d_grid, d_ff, G.dev<int>(o_msin), M.where, stamp, t->T.capacity, d_flag, d_oct, d_ms, d_found);
        };
        marks();
        LoopArgs A{};
        A.n_kf = n_kf; A.n_points = n_pt; A.views = M.views; A.slot = d_slot; A.held = d_held; A.found = d_found;
        A.log_scale = p->log_scale_factor; A.n_levels = p->n_levels; A.th = p->th;
        fill_levels(A.scale, p->scale_factors, p->n_levels);
        A.qx = (float*)(wk + w_qx); A.qy = (float*)(wk + w_qy); A.qr = (float*)(wk + w_qr); A.none = (int*)(wk + w_none); A.qkf = (int*)(wk + w_qkf);
        A.qlevel = (int*)(wk + w_qlvl); A.act = wk + w_act; A.qdesc = wk + w_qdesc; A.out = d_out;
        A.gate = r->gate ? G.dev<uint8_t>(o_gate) : nullptr;
        A.u = taps ? G.dev<float>(o_u) : nullptr; A.v = taps ? G.dev<float>(o_v) : nullptr; A.level = taps ? G.dev<int>(o_lvl) : nullptr;
        loop_launch_project(st, A, t->T);
        CCM_HIP(c, hipGetLastError());
        const WinLists L{ WinGrid{}, d_grid, A.qkf, (int)m, A.qx, A.qy, A.qr, A.none, A.none, A.qdesc, &S.ci, &S.cd, &S.cn };
        auto deliver = [&]() {
            G.get(r->best_idx, o_bi, m * 4); G.get(r->observed, o_obs, m); G.get(r->matched_slot, o_ms, NF * 4);
            G.get(r->best_dist, o_bd, m * 4); G.get(r->gate, o_gate, m);
            G.get(r->u, o_u, m * 4); G.get(r->v, o_v, m * 4); G.get(r->level, o_lvl, m * 4);
        };

        if (NF == 0) {                                                         // no view has features: every surviving pair is EMPTY_KF
            if (r->best_dist) loop_launch_finish(st, n_kf, n_pt, d_grid, d_ff, d_slot, d_out, d_held, t->T, d_ms, G.dev<int>(o_bd));
            if ((rc = G.download(c, 0, res_end)) || (rc = G.wait(c))) return rc;
            deliver();
            for (int k = 0; k < n_kf; k++) r->n_matches[k] = 0;
            return 0;
        }
        if (!window_host_accept_forced() && match_window_greedy_lds(max_n, 0) <= kGreedyLdsMax) {
            GreedyArgs Q{ 0, 0, 0, nullptr, nullptr, nullptr, A.act, A.qlevel, d_oct, d_held, d_flag, 0.f, d_out, d_status,
                          0, 0, nullptr, nullptr, nullptr, G.dev<GreedyKf>(o_gk) };
            // the first attempt may have set flags and choices in the views whose lists fitted
            auto reset = [&]() -> int { marks(); CCM_HIP(c, hipMemsetAsync(d_out, 0xFF, m * 4, st)); return CCM_OK; };
            auto tail = [&] { loop_launch_finish(st, n_kf, n_pt, d_grid, d_ff, d_slot, d_out, d_held, t->T, d_ms, r->best_dist ? G.dev<int>(o_bd) : nullptr); };
            // the one synchronisation
            auto fetch = [&](const int** s) -> int { *s = G.host<int>(o_status); const int e = G.download(c, 0, res_end); return e ? e : G.wait(c); };
            const int* status = nullptr;
            if ((rc = window_greedy_drive(c, L, Q, 1, n_kf, max_n, reset, tail, fetch, &status))) return rc;
            deliver();
            int total = 0;
            for (int k = 0; k < n_kf; k++) { r->n_matches[k] = status[3 * k]; total += status[3 * k]; }
            return total;
        }

        // host acceptance (CCM_WINDOW_HOST_ACCEPT=1, or a handle too large for the acceptance kernel's LDS): the lists, the queries' flags
        // and the octaves come to the host, and window_accept_sim3_host runs there, view by view
        WinHostLists H{ 64 };
        std::vector<int32_t> qlvl(m), oct(NF);
        std::vector<uint8_t> act(m), matched;
        if ((rc = window_lists_host(c, L, H))) return rc;
        if ((rc = frame_fetch(c, qlvl.data(), A.qlevel, m * 4)) || (rc = frame_fetch(c, act.data(), A.act, m)) ||
            (rc = frame_fetch(c, oct.data(), d_oct, NF * 4))) return rc;
        if ((rc = G.download(c, 0, res_end)) || (rc = G.wait(c))) return rc;
        int* bi = G.host<int>(o_bi); int* ms = G.host<int>(o_ms); const uint8_t* held = G.host<uint8_t>(o_obs);
        int* bd = r->best_dist ? G.host<int>(o_bd) : nullptr;
        int total = 0;
        for (int k = 0; k < n_kf; k++) {
            const size_t q0 = (size_t)k * n_pt;
            matched.resize(ff[k + 1] - ff[k]);                                 // vpMatched as flags ...
            for (int i = ff[k]; i < ff[k + 1]; i++) matched[i - ff[k]] = ms[i] >= 0;
            r->n_matches[k] = window_accept_sim3_host(n_pt, act.data() + q0, qlvl.data() + q0, H.ci.data() + q0 * H.cap, H.cd.data() + q0 * H.cap, H.cn.data() + q0, H.cap,
                                                      oct.data() + ff[k], held + q0, matched.data(), bi + q0, bd ? bd + q0 : nullptr);
            for (int j = 0; j < n_pt; j++)                                     // ... and the accepted, unobserved points as slots (:436-440)
                if (bi[q0 + j] >= 0 && !held[q0 + j]) ms[ff[k] + bi[q0 + j]] = p->slot[j];
            total += r->n_matches[k];
        }
        deliver();
        return total;
    });
}

}  // extern "C"
