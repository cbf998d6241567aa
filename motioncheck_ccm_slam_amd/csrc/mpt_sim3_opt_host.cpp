// mpt_sim3_opt_host.cpp -- ComputeSim3's solver and optimiser on keyframe handles and the map-point table (include/ccm_hot.h
// "ComputeSim3 on handles: the solver, OptimizeSim3 and the chain"): ccm_sim3_solver_create_frames and ccm_optimize_sim3_table_frames
// put a gather kernel in front of the unchanged k_sim3_ransac and k_sim3_opt, and ccm_compute_sim3_table_frames queues the list, the
// gather, k_sim3_opt and the scatter behind the pipeline of ccm_search_by_sim3_table_frames (mpt_sim3_host.cpp).  The arrays k_sim3_opt
// reads are the context's Sim3State, as for ccm_optimize_sim3; everything small stages through the frame handles' block.
#include "mpt_internal.h"
#include "sim3_internal.h"

static_assert(sizeof(Sim3FramesPair) == 168, "per-pair upload of the calls of mpt_sim3_opt_host.cpp");

// A pair of the caller's: CCM_E_ARG for a null handle or one of another context, CCM_E_STATE for one that outlived its context
static int frames_pair_check(ccm_ctx* c, const ccm_frame* k1, const ccm_frame* k2, const char* fn, int k)
{
    if (!k1 || !k2) return ccm_fail(c, CCM_E_ARG, "%s: null pairs[%d].%s", fn, k, !k1 ? "kf1" : "kf2");
    int rc;
    if ((rc = frame_named_check(c, k1, CCM_E_STATE, fn, "pairs[%d].kf1", k)) || (rc = frame_named_check(c, k2, CCM_E_STATE, fn, "pairs[%d].kf2", k))) return rc;
    return CCM_OK;
}
static bool levels_ok(int n) { return n >= 1 && n <= CCM_MAX_LEVELS; }

// The buffers of k_sim3_opt for `rows` correspondences, from the context's Sim3State
static int opt_buffers(ccm_ctx* c, size_t rows, Sim3State** out)
{
    if (!c->sim3) c->sim3 = new Sim3State();
    Sim3State& S = *c->sim3;
    const size_t n = std::max<size_t>(rows, 2);
    CCM_RESERVE(c, S.P1, n * 24); CCM_RESERVE(c, S.P2, n * 24); CCM_RESERVE(c, S.o1, n * 16); CCM_RESERVE(c, S.o2, n * 16);
    CCM_RESERVE(c, S.i1, n * 8); CCM_RESERVE(c, S.i2, n * 8); CCM_RESERVE(c, S.err, n * 32); CCM_RESERVE(c, S.inl, n);
    *out = &S;
    return CCM_OK;
}

extern "C" {

int ccm_sim3_solver_create_frames(ccm_ctx* c, ccm_map_table* t, const ccm_sim3_solver_frames_problem* p, ccm_sim3_solver** out)
{
    RoctxRange roctx_("ccm_sim3_solver_create_frames");
    if (!c || !t || !p || !out) return CCM_E_ARG;
    const char* fn = "ccm_sim3_solver_create_frames";
    int rc = check_table(c, t);
    if (rc) return rc;
    if (p->n_solvers < 0 || !levels_ok(p->n_levels1) || !levels_ok(p->n_levels2) || !p->max_err_level1 || !p->max_err_level2)
        return ccm_fail(c, CCM_E_ARG, "%s: n_solvers = %d, n_levels = %d, %d (1..%d), max_err_level1 / 2 %s", fn, p->n_solvers, p->n_levels1, p->n_levels2,
                        CCM_MAX_LEVELS, p->max_err_level1 && p->max_err_level2 ? "given" : "null");
    if (p->n_solvers > 0 && (!p->pairs || !p->first)) return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !p->pairs ? "pairs" : "first");
    const int F = p->n_solvers;
    if (F > 0 && p->first[F] > 0 && (!p->feature1 || !p->feature2)) return ccm_fail(c, CCM_E_ARG, "%s: null correspondence array", fn);
    return table_call(c, t, false, fn, [&]() -> int {                       // reads pos and flags
        std::vector<Sim3FramesPair> views((size_t)F);
        std::vector<int32_t> n1((size_t)std::max(F, 1));
        std::vector<float> K((size_t)std::max(F, 1) * 8);
        for (int k = 0; k < F; k++) {
            const ccm_sim3_frames_pair& P = p->pairs[k];
            if ((rc = frames_pair_check(c, P.kf1, P.kf2, fn, k))) return rc;
            views[k] = sim3_frames_pair(P.kf1, P.kf2, P.T1w, P.T2w);
            n1[k] = P.kf1->n;                                               // mN1 = vpMatched12.size() = pKF1's N
            std::memcpy(&K[4 * (size_t)k], P.K1, 16); std::memcpy(&K[4 * ((size_t)F + k)], P.K2, 16);
        }
        const ccm_sim3_ransac_problem pb{ F, p->first, n1.data(), p->fix_scale, K.data(), K.data() + 4 * (size_t)F, nullptr, nullptr, nullptr, nullptr,
                                          p->feature1, p->probability, p->min_inliers, p->max_iterations, p->draws, p->best_inliers };
        const Sim3SolverFrames fr{ t->T, views.data(), p->feature1, p->feature2, p->max_err_level1, p->max_err_level2, p->n_levels1, p->n_levels2 };
        return sim3_solver_create_body(c, &pb, &fr, out);
    });
}

// Staging: [ n_inliers | inlier | status | sim3 ] down, [ status | sim3 | K1 | K2 | first | fix_scale | th2 | pairs | feature1 |
// feature2 | level tables ] up: sim3 goes both ways, the status word goes up as zero.
int ccm_optimize_sim3_table_frames(ccm_ctx* c, ccm_map_table* t, const ccm_sim3_opt_frames_problem* p, ccm_sim3_opt_frames_result* r)
{
    RoctxRange roctx_("ccm_optimize_sim3_table_frames");
    if (!c || !t || !p || !r) return CCM_E_ARG;
    const char* fn = "ccm_optimize_sim3_table_frames";
    int rc = check_table(c, t);
    if (rc) return rc;
    if (p->n_problems < 0) return ccm_fail(c, CCM_E_ARG, "%s: n_problems = %d", fn, p->n_problems);
    if (p->n_problems == 0) return CCM_OK;
    if (!p->pairs || !p->first || !p->fix_scale || !p->th2 || !p->inv_level_sigma2_1 || !p->inv_level_sigma2_2 || !r->sim3 || !r->n_inliers)
        return ccm_fail(c, CCM_E_ARG, "%s: null per-problem array or level table", fn);
    if (!levels_ok(p->n_levels1) || !levels_ok(p->n_levels2))
        return ccm_fail(c, CCM_E_ARG, "%s: n_levels = %d, %d outside 1..%d", fn, p->n_levels1, p->n_levels2, CCM_MAX_LEVELS);
    const int F = p->n_problems;
    if (p->first[0] != 0) return ccm_fail(c, CCM_E_ARG, "%s: first[0] must be 0", fn);
    int max_n = 0;
    for (int k = 0; k < F; k++) {
        if (p->first[k + 1] < p->first[k]) return ccm_fail(c, CCM_E_ARG, "%s: first[] must be non-decreasing", fn);
        max_n = std::max(max_n, p->first[k + 1] - p->first[k]);
    }
    const size_t T = (size_t)p->first[F];
    if (T > 0 && (!p->feature1 || !p->feature2 || !r->inlier)) return ccm_fail(c, CCM_E_ARG, "%s: null correspondence array", fn);
    return table_call(c, t, false, fn, [&]() -> int {                       // reads pos and flags
        for (int k = 0; k < F; k++)
            if ((rc = frames_pair_check(c, p->pairs[k].kf1, p->pairs[k].kf2, fn, k))) return rc;
        CCM_HIP(c, hipSetDevice(c->device));
        Staging& G = frame_state(c)->stage;
        hipStream_t st = c->stream;
        Sim3State* S = nullptr;
        if ((rc = opt_buffers(c, T, &S))) return rc;
        size_t off = 0;
        const size_t o_nin = seg(off, (size_t)F * 4), o_inl = seg(off, T), o_status = seg(off, 16), o_sim3 = seg(off, (size_t)F * 64);
        const size_t res_end = off;
        const size_t o_K1 = seg(off, (size_t)F * 32), o_K2 = seg(off, (size_t)F * 32), o_first = seg(off, ((size_t)F + 1) * 4), o_fix = seg(off, (size_t)F * 4);
        const size_t o_th2 = seg(off, (size_t)F * 4), o_view = seg(off, (size_t)F * sizeof(Sim3FramesPair)), o_f1 = seg(off, T * 4), o_f2 = seg(off, T * 4);
        const size_t o_t1 = seg(off, CCM_MAX_LEVELS * 4), o_t2 = seg(off, CCM_MAX_LEVELS * 4);
        const size_t end = off;
        if ((rc = G.reserve(c, end))) return rc;
        std::memset(G.host<uint8_t>(o_status), 0, 16);
        G.put(o_sim3, r->sim3, (size_t)F * 64);
        double* K1 = G.host<double>(o_K1); double* K2 = G.host<double>(o_K2);
        Sim3FramesPair* hv = G.host<Sim3FramesPair>(o_view);
        for (int k = 0; k < F; k++) {
            const ccm_sim3_frames_pair& P = p->pairs[k];
            for (int i = 0; i < 4; i++) { K1[4 * k + i] = (double)P.K1[i]; K2[4 * k + i] = (double)P.K2[i]; }       // :895-902
            hv[k] = sim3_frames_pair(P.kf1, P.kf2, P.T1w, P.T2w);
        }
        G.put(o_first, p->first, ((size_t)F + 1) * 4); G.put(o_fix, p->fix_scale, (size_t)F * 4); G.put(o_th2, p->th2, (size_t)F * 4);
        G.put(o_f1, p->feature1, T * 4); G.put(o_f2, p->feature2, T * 4);
        G.put(o_t1, p->inv_level_sigma2_1, (size_t)p->n_levels1 * 4); G.put(o_t2, p->inv_level_sigma2_2, (size_t)p->n_levels2 * 4);
        if ((rc = G.upload(c, o_status, end))) return rc;
        sim3_opt_gather_launch(st, Sim3OptGather{ G.dev<Sim3FramesPair>(o_view), G.dev<int>(o_first), G.dev<int>(o_f1), G.dev<int>(o_f2), p->n_levels1, p->n_levels2,
                                                  G.dev<float>(o_t1), G.dev<float>(o_t2), S->P1.as<double>(), S->P2.as<double>(), S->o1.as<double>(),
                                                  S->o2.as<double>(), S->i1.as<double>(), S->i2.as<double>(), G.dev<int>(o_status) }, t->T, F, max_n);
        sim3_launch(st, Sim3Dev{ F, G.dev<double>(o_sim3), G.dev<int>(o_fix), G.dev<double>(o_K1), G.dev<double>(o_K2), G.dev<int>(o_first), S->P1.as<double>(),
                                 S->P2.as<double>(), S->o1.as<double>(), S->o2.as<double>(), S->i1.as<double>(), S->i2.as<double>(), G.dev<float>(o_th2),
                                 S->err.as<double>(), G.dev<uint8_t>(o_inl), G.dev<int>(o_nin) });
        CCM_HIP(c, hipGetLastError());
        if ((rc = G.download(c, 0, res_end)) || (rc = G.wait(c))) return rc;
        if (*G.host<int32_t>(o_status))
            return ccm_fail(c, CCM_E_ARG, "%s: a correspondence names a feature outside its handle, a slot that is not LIVE or an octave outside [0, %d) / [0, %d)",
                            fn, p->n_levels1, p->n_levels2);
        G.get(r->sim3, o_sim3, (size_t)F * 64); G.get(r->inlier, o_inl, T); G.get(r->n_inliers, o_nin, (size_t)F * 4);
        return CCM_OK;
    });
}

int ccm_compute_sim3_table_frames(ccm_ctx* c, ccm_map_table* t, const ccm_compute_sim3_problem* p, ccm_compute_sim3_result* r)
{
    RoctxRange roctx_("ccm_compute_sim3_table_frames");
    if (!c || !t || !p || !r) return CCM_E_ARG;
    const char* fn = "ccm_compute_sim3_table_frames";
    if (p->n_pairs > 0 && !p->pairs) { int rc = check_table(c, t); return rc ? rc : ccm_fail(c, CCM_E_ARG, "%s: null pairs", fn); }
    return ccm_guard(c, fn, [&]() -> int {
        std::vector<ccm_sim3_search_pair> sp((size_t)std::max(p->n_pairs, 0));
        for (int k = 0; k < p->n_pairs; k++) sp[k] = p->pairs[k].search;
        const ccm_sim3_search_problem q{ p->n_pairs, sp.data(), p->th, p->log_scale_factor1, p->n_levels1, p->scale_factors1,
                                         p->log_scale_factor2, p->n_levels2, p->scale_factors2 };
        int rc = sim3_search_check(c, t, &q, &r->search, fn);
        if (rc || p->n_pairs == 0) return rc;
        if (!p->inv_level_sigma2_1 || !p->inv_level_sigma2_2 || !r->n_correspondences || !r->n_inliers || !r->sim3)
            return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !p->inv_level_sigma2_1 || !p->inv_level_sigma2_2 ? "inv_level_sigma2_1 / 2" : "n_correspondences / n_inliers / sim3");
        Sim3Chain chain{ p, r };
        return table_call(c, t, false, fn, [&]() -> int {
            size_t sum1 = 0;
            for (int k = 0; k < p->n_pairs; k++) {                          // what the search does not ask of a pair
                const ccm_sim3_search_pair& P = sp[k];
                if ((rc = frames_pair_check(c, P.kf1, P.kf2, fn, k))) return rc;
                if (P.kf1->n_levels > p->n_levels1 || P.kf2->n_levels > p->n_levels2)
                    return ccm_fail(c, CCM_E_ARG, "%s: pairs[%d] has octaves up to %d, %d; n_levels = %d, %d", fn, k, P.kf1->n_levels - 1, P.kf2->n_levels - 1,
                                    p->n_levels1, p->n_levels2);
                sum1 += (size_t)P.kf1->n;
            }
            if (sum1 > 0 && !r->pruned) return ccm_fail(c, CCM_E_ARG, "%s: null pruned", fn);
            return sim3_search_run(c, t, &q, &r->search, fn, &chain);
        });
    });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------- the chain's half
// Result segment: [ pruned | first | n_inliers | status | (feature1 | feature2) | (inlier) ], the lists only when tapped; input
// segment: [ sim3 | K1 | K2 | fix_scale | th2 | views | level tables ]; work: [ cnt | feature1 | feature2 | inlier ] where not tapped.
void Sim3Chain::size(int P, size_t s1)
{
    n_pairs = P; sum1 = s1;
    const size_t rows = std::max<size_t>(sum1, 1);
    size_t off = 0;
    r_pruned = seg(off, sum1); r_first = seg(off, ((size_t)P + 1) * 4); r_nin = seg(off, (size_t)P * 4); r_status = seg(off, 16);
    r_f1 = seg(off, r->corr ? rows * 4 : 0); r_f2 = seg(off, r->corr ? rows * 4 : 0); r_inl = seg(off, r->inlier ? rows : 0);
    res_bytes = off;
    off = 0;
    i_sim3 = seg(off, (size_t)P * 64); i_K1 = seg(off, (size_t)P * 32); i_K2 = seg(off, (size_t)P * 32); i_fix = seg(off, (size_t)P * 4);
    i_th2 = seg(off, (size_t)P * 4); i_view = seg(off, (size_t)P * sizeof(Sim3FramesPair)); i_t1 = seg(off, CCM_MAX_LEVELS * 4); i_t2 = seg(off, CCM_MAX_LEVELS * 4);
    in_bytes = off;
    off = 0;
    w_cnt = seg(off, (size_t)P * 4); w_f1 = seg(off, r->corr ? 0 : rows * 4); w_f2 = seg(off, r->corr ? 0 : rows * 4); w_inl = seg(off, r->inlier ? 0 : rows);
    work_bytes = off;
}

void Sim3Chain::fill(Staging& G, size_t o) const
{
    double* s3 = G.host<double>(o + i_sim3); double* K1 = G.host<double>(o + i_K1); double* K2 = G.host<double>(o + i_K2);
    int32_t* fix = G.host<int32_t>(o + i_fix); float* th2 = G.host<float>(o + i_th2);
    Sim3FramesPair* hv = G.host<Sim3FramesPair>(o + i_view);
    for (int k = 0; k < n_pairs; k++) {
        const ccm_compute_sim3_pair& P = p->pairs[k];
        std::memcpy(s3 + 8 * (size_t)k, P.sim3, 64);
        const float k1[4] = { P.search.fx, P.search.fy, P.search.cx, P.search.cy };
        for (int i = 0; i < 4; i++) { K1[4 * k + i] = (double)k1[i]; K2[4 * k + i] = (double)P.K2[i]; }
        fix[k] = P.fix_scale; th2[k] = P.th2;
        hv[k] = sim3_frames_pair(P.search.kf1, P.search.kf2, P.search.T1w, P.search.T2w);
    }
    G.put(o + i_t1, p->inv_level_sigma2_1, (size_t)p->n_levels1 * 4); G.put(o + i_t2, p->inv_level_sigma2_2, (size_t)p->n_levels2 * 4);
}

int Sim3Chain::queue(ccm_ctx* c, const MptTable& T, Staging& G, size_t o_res, size_t o_in, uint8_t* work, int max_n1, const Sim3Pair* d_pair,
                     const int* d_matched12, const int* d_matched_idx2, const int* d_match12) const
{
    hipStream_t st = c->stream;
    Sim3State* S = nullptr;
    int rc = opt_buffers(c, sum1, &S);
    if (rc) return rc;
    int* f1 = r->corr ? G.dev<int>(o_res + r_f1) : (int*)(work + w_f1); int* f2 = r->corr ? G.dev<int>(o_res + r_f2) : (int*)(work + w_f2);
    uint8_t* inl = r->inlier ? G.dev<uint8_t>(o_res + r_inl) : work + w_inl;
    int* first = G.dev<int>(o_res + r_first); int* status = G.dev<int>(o_res + r_status);
    uint8_t* pruned = G.dev<uint8_t>(o_res + r_pruned);
    const Sim3FramesPair* views = G.dev<Sim3FramesPair>(o_in + i_view);
    if (sum1) CCM_HIP(c, hipMemsetAsync(pruned, 0, sum1, st));
    CCM_HIP(c, hipMemsetAsync(status, 0, 16, st));
    const Sim3ChainArgs A{ n_pairs, (int)sum1, d_pair, views, d_matched12, d_matched_idx2, d_match12, (int*)(work + w_cnt), first, f1, f2 };
    sim3_chain_list_launch(st, A, T);
    sim3_opt_gather_launch(st, Sim3OptGather{ views, first, f1, f2, p->n_levels1, p->n_levels2, G.dev<float>(o_in + i_t1), G.dev<float>(o_in + i_t2),
                                              S->P1.as<double>(), S->P2.as<double>(), S->o1.as<double>(), S->o2.as<double>(), S->i1.as<double>(),
                                              S->i2.as<double>(), status }, T, n_pairs, max_n1);
    sim3_launch(st, Sim3Dev{ n_pairs, G.dev<double>(o_in + i_sim3), G.dev<int>(o_in + i_fix), G.dev<double>(o_in + i_K1), G.dev<double>(o_in + i_K2), first,
                             S->P1.as<double>(), S->P2.as<double>(), S->o1.as<double>(), S->o2.as<double>(), S->i1.as<double>(), S->i2.as<double>(),
                             G.dev<float>(o_in + i_th2), S->err.as<double>(), inl, G.dev<int>(o_res + r_nin) });
    sim3_chain_scatter_launch(st, A, max_n1, inl, pruned);
    CCM_HIP(c, hipGetLastError());
    return G.download(c, o_in + i_sim3, o_in + i_sim3 + (size_t)n_pairs * 64);
}

int Sim3Chain::deliver(ccm_ctx* c, const Staging& G, size_t o_res, size_t o_in) const
{
    if (*G.host<int32_t>(o_res + r_status)) return ccm_fail(c, CCM_E_DEVICE, "ccm_compute_sim3_table_frames: a listed correspondence did not resolve");
    const int32_t* first = G.host<int32_t>(o_res + r_first);
    for (int k = 0; k < n_pairs; k++) r->n_correspondences[k] = first[k + 1] - first[k];
    const size_t rows = (size_t)first[n_pairs];
    G.get(r->pruned, o_res + r_pruned, sum1); G.get(r->n_inliers, o_res + r_nin, (size_t)n_pairs * 4); G.get(r->sim3, o_in + i_sim3, (size_t)n_pairs * 64);
    if (r->corr) {
        const int32_t* f1 = G.host<int32_t>(o_res + r_f1); const int32_t* f2 = G.host<int32_t>(o_res + r_f2);
        for (size_t e = 0; e < rows; e++) { r->corr[2 * e] = f1[e]; r->corr[2 * e + 1] = f2[e]; }
    }
    G.get(r->inlier, o_res + r_inl, rows);
    return CCM_OK;
}

void Sim3Chain::none() const
{
    for (int k = 0; k < p->n_pairs; k++) {
        r->n_correspondences[k] = 0; r->n_inliers[k] = 0;
        std::memcpy(r->sim3 + 8 * (size_t)k, p->pairs[k].sim3, 64);
    }
}
