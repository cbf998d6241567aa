// sim3_ransac_host.cpp -- C ABI of the batched Sim3Solver (src/Sim3Solver.cpp): create evaluates every hypothesis of every solver in
// one kernel launch (sim3_ransac_kernels.hip); iterate / find replay the ordered bookkeeping of Sim3Solver::iterate (:120-191) over
// the stored per-hypothesis counts on the host.
#include "sim3_internal.h"
#include <cmath>
#include <memory>

void sim3_ransac_state_free(Sim3RansacState* s)
{
    if (!s) return;
    s->stage.release();
    delete s;
}

struct S3rHost {                  // one Sim3Solver
    int n = 0, n1 = 0;            // N, mN1
    int hyp_first = 0, n_hyp = 0, words = 0;
    size_t first = 0, mask_first = 0;
    int max_its = 1;              // mRansacMaxIts
    int iterations = 0;           // mnIterations
    int best_inliers = 0;         // mnBestInliers
    int best = -1;                // hypothesis behind mBestT12 / mBestRotation / ..., -1 = none yet
};
struct ccm_sim3_solver {
    int min_inliers = 0;
    std::vector<S3rHost> k;
    std::vector<int32_t> indices1, count, sample;
    std::vector<float> rts;
    std::vector<uint64_t> mask;
};

extern "C" int ccm_sim3_ransac_iterations(int n, double probability, int min_inliers, int max_iterations)
{
    if (n <= 0 || n < min_inliers) return 1;                                // undefined in the reference and never used (:129)
    int it;
    if (min_inliers == n) it = 1;                                           // :110-113
    else {
        const float epsilon = (float)min_inliers / n;
        const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow(epsilon, 3)));
        it = v >= (double)max_iterations ? max_iterations : (v >= 1 ? (int)v : 1);    // the conversion stays inside int's range
    }
    return std::max(1, std::min(it, max_iterations));                       // :115
}

int sim3_solver_create_body(ccm_ctx* c, const ccm_sim3_ransac_problem* pb, const Sim3SolverFrames* fr, ccm_sim3_solver** out)
{
    if (!pb || !out || pb->n_solvers < 0) return ccm_fail(c, CCM_E_ARG, "bad Sim3 RANSAC problem");
    const int F = pb->n_solvers;
    std::unique_ptr<ccm_sim3_solver> S(new ccm_sim3_solver());
    S->min_inliers = pb->min_inliers;
    if (F == 0) { *out = S.release(); return CCM_OK; }
    if (!pb->first || !pb->n1 || !pb->fix_scale || !pb->K1 || !pb->K2) return ccm_fail(c, CCM_E_ARG, "bad Sim3 RANSAC problem: null per-solver array");
    if (pb->max_iterations < 1 || pb->min_inliers < 0) return ccm_fail(c, CCM_E_ARG, "bad RANSAC parameters: max_iterations %d, min_inliers %d", pb->max_iterations, pb->min_inliers);
    if (pb->first[0] != 0) return ccm_fail(c, CCM_E_ARG, "first[0] must be 0");
    for (int f = 0; f < F; f++) if (pb->first[f + 1] < pb->first[f]) return ccm_fail(c, CCM_E_ARG, "first[] must be non-decreasing");
    const size_t T = (size_t)pb->first[F];
    if (T > 0 && (!pb->indices1 || (fr ? !fr->feature2 : (!pb->X1 || !pb->X2 || !pb->max_err1 || !pb->max_err2))))
        return ccm_fail(c, CCM_E_ARG, "bad Sim3 RANSAC problem: null correspondence array");

    // ---- per-solver geometry of the batch, and the checks that keep every index the kernel and iterate() form in range
    S->k.resize(F);
    size_t H = 0, W = 0, n_blocks = 0;
    for (int f = 0; f < F; f++) {
        S3rHost& k = S->k[f];
        k.first = (size_t)pb->first[f]; k.n = pb->first[f + 1] - pb->first[f]; k.n1 = pb->n1[f];
        if (k.n1 < 0) return ccm_fail(c, CCM_E_ARG, "solver %d: n1 = %d", f, k.n1);
        for (int i = 0; i < k.n; i++) {
            const int32_t i1 = pb->indices1[k.first + i];
            if (i1 < 0 || i1 >= k.n1) return ccm_fail(c, CCM_E_ARG, "solver %d: indices1[%d] = %d outside [0, %d)", f, i, i1, k.n1);
        }
        k.max_its = ccm_sim3_ransac_iterations(k.n, pb->probability, pb->min_inliers, pb->max_iterations);
        k.best_inliers = pb->best_inliers ? pb->best_inliers[f] : 0;
        k.n_hyp = (k.n >= 3 && k.n >= pb->min_inliers) ? k.max_its : 0;
        k.words = (k.n + 63) / 64;
        k.hyp_first = (int)H; k.mask_first = W;
        H += (size_t)k.n_hyp; W += (size_t)k.n_hyp * k.words;
        n_blocks += ((size_t)k.n_hyp + S3R_HPB - 1) / S3R_HPB;
        if (H > (size_t)INT32_MAX / 16) return ccm_fail(c, CCM_E_ARG, "too many hypotheses in one batch");
    }
    if (H > 0 && !pb->draws) return ccm_fail(c, CCM_E_ARG, "bad Sim3 RANSAC problem: null draws");
    for (int f = 0; f < F; f++) {
        const S3rHost& k = S->k[f];
        const int32_t* d = pb->draws + (size_t)f * pb->max_iterations * 3;
        for (int h = 0; h < k.n_hyp; h++)
            for (int i = 0; i < 3; i++)
                if (d[3 * h + i] < 0 || d[3 * h + i] > k.n - 1 - i)
                    return ccm_fail(c, CCM_E_ARG, "solver %d, hypothesis %d: draw %d = %d outside [0, %d]", f, h, i, d[3 * h + i], k.n - 1 - i);
    }
    S->indices1.assign(pb->indices1, pb->indices1 + T);
    if (H == 0) { *out = S.release(); return CCM_OK; }                  // nothing to evaluate: every solver reports bNoMore

    // ---- staging: [solvers | blocks | draws | X1 | X2 | bounds] up, [status | count | sample | rts | mask] down.  With frames
    // [pairs | feature1 | feature2 | level tables] go up in the place of X1 | X2 | bounds, which k_sim3_solver_gather fills on the device.
    size_t off = 0;
    const size_t o_solvers = seg(off, (size_t)F * sizeof(S3rSolver)), o_blocks = seg(off, n_blocks * sizeof(S3rBlock)), o_draws = seg(off, H * 12);
    const size_t o_pairs = seg(off, fr ? (size_t)F * sizeof(Sim3FramesPair) : 0), o_f1 = seg(off, fr ? T * 4 : 0), o_f2 = seg(off, fr ? T * 4 : 0);
    const size_t o_t1 = seg(off, fr ? CCM_MAX_LEVELS * 4 : 0), o_t2 = seg(off, fr ? CCM_MAX_LEVELS * 4 : 0);
    const size_t up_end = off;                                          // with frames: the end of the upload
    const size_t o_x1 = seg(off, T * 12), o_x2 = seg(off, T * 12), o_m1 = seg(off, T * 4), o_m2 = seg(off, T * 4);
    const size_t in_end = off;
    const size_t o_status = seg(off, 16);
    const size_t o_count = seg(off, H * 4), o_sample = seg(off, H * 12), o_rts = seg(off, H * 52), o_mask = seg(off, W * 8);
    const size_t end = off;
    CCM_HIP(c, hipSetDevice(c->device));
    if (!c->sim3_ransac) c->sim3_ransac = new Sim3RansacState();
    Staging& G = c->sim3_ransac->stage;
    int rc;
    if ((rc = G.reserve(c, end))) return rc;
    S3rSolver* hs = G.host<S3rSolver>(o_solvers);
    S3rBlock* hb = G.host<S3rBlock>(o_blocks);
    size_t nb = 0;
    int max_n = 0;
    for (int f = 0; f < F; f++) {
        const S3rHost& k = S->k[f];
        S3rSolver& s = hs[f];
        s.first = (int32_t)k.first; s.n = k.n; s.fix_scale = pb->fix_scale[f]; s.hyp_first = k.hyp_first; s.n_hyp = k.n_hyp;
        s.words = k.words; s.mask_first = (int64_t)k.mask_first;
        std::memcpy(s.K1, pb->K1 + 4 * f, 16); std::memcpy(s.K2, pb->K2 + 4 * f, 16);
        for (int h0 = 0; h0 < k.n_hyp; h0 += S3R_HPB) hb[nb++] = S3rBlock{ f, h0, std::min(S3R_HPB, k.n_hyp - h0), 0 };
        G.put(o_draws + (size_t)k.hyp_first * 12, pb->draws + (size_t)f * pb->max_iterations * 3, (size_t)k.n_hyp * 12);
        max_n = std::max(max_n, k.n);
    }
    const S3rDev D{ G.dev<S3rSolver>(o_solvers), G.dev<S3rBlock>(o_blocks), G.dev<float>(o_x1), G.dev<float>(o_x2), G.dev<float>(o_m1),
                    G.dev<float>(o_m2), G.dev<int32_t>(o_draws), G.dev<int32_t>(o_count), G.dev<int32_t>(o_sample), G.dev<float>(o_rts),
                    G.dev<unsigned long long>(o_mask) };
    if (fr) {
        G.put(o_pairs, fr->pairs, (size_t)F * sizeof(Sim3FramesPair));
        G.put(o_f1, fr->feature1, T * 4); G.put(o_f2, fr->feature2, T * 4);
        G.put(o_t1, fr->max_err_level1, (size_t)fr->n_levels1 * 4); G.put(o_t2, fr->max_err_level2, (size_t)fr->n_levels2 * 4);
        if ((rc = G.upload(c, 0, up_end))) return rc;
        CCM_HIP(c, hipMemsetAsync(G.dev<int32_t>(o_status), 0, 16, c->stream));
        sim3_solver_gather_launch(c->stream, Sim3SolverGather{ G.dev<Sim3FramesPair>(o_pairs), D.solvers, G.dev<int32_t>(o_f1), G.dev<int32_t>(o_f2),
                                                               fr->n_levels1, fr->n_levels2, G.dev<float>(o_t1), G.dev<float>(o_t2),
                                                               G.dev<float>(o_x1), G.dev<float>(o_x2), G.dev<float>(o_m1), G.dev<float>(o_m2),
                                                               G.dev<int32_t>(o_status) }, fr->T, F, max_n);
        CCM_HIP(c, hipGetLastError());
    } else {
        G.put(o_x1, pb->X1, T * 12); G.put(o_x2, pb->X2, T * 12);
        G.put(o_m1, pb->max_err1, T * 4); G.put(o_m2, pb->max_err2, T * 4);
        if ((rc = G.upload(c, 0, in_end))) return rc;
    }
    sim3_ransac_launch(c->stream, D, (int)n_blocks);
    CCM_HIP(c, hipGetLastError());
    if ((rc = G.download(c, fr ? o_status : o_count, end)) || (rc = G.wait(c))) return rc;
    if (fr && *G.host<int32_t>(o_status))
        return ccm_fail(c, CCM_E_ARG, "a correspondence names a feature outside its handle, a slot that is not LIVE or an octave outside [0, %d) / [0, %d)",
                        fr->n_levels1, fr->n_levels2);
    const int32_t* rn = G.host<int32_t>(o_count); const int32_t* rs = G.host<int32_t>(o_sample);
    const float* rr = G.host<float>(o_rts); const uint64_t* rm = G.host<uint64_t>(o_mask);
    S->count.assign(rn, rn + H); S->sample.assign(rs, rs + 3 * H); S->rts.assign(rr, rr + 13 * H); S->mask.assign(rm, rm + W);
    *out = S.release();
    return CCM_OK;
}

extern "C" int ccm_sim3_solver_create(ccm_ctx* c, const ccm_sim3_ransac_problem* pb, ccm_sim3_solver** out)
{
    RoctxRange roctx_("ccm_sim3_solver_create");
    return ccm_guard(c, "ccm_sim3_solver_create", [&]() -> int {
        if (!c) return CCM_E_ARG;
        return sim3_solver_create_body(c, pb, nullptr, out);
    });
}

extern "C" void ccm_sim3_solver_destroy(ccm_sim3_solver* s) { delete s; }

extern "C" int ccm_sim3_solver_count(const ccm_sim3_solver* s) { return s ? (int)s->k.size() : CCM_E_ARG; }

// mBestT12 of hypothesis h: [sR | t; 0 0 0 1] (:305-310), the products the kernel formed
static void t12_of(const float* rts, float* T12)
{
    for (int r = 0; r < 3; r++) {
        for (int col = 0; col < 3; col++) T12[4 * r + col] = rts[12] * rts[3 * r + col];
        T12[4 * r + 3] = rts[9 + r];
    }
    T12[12] = T12[13] = T12[14] = 0.0f; T12[15] = 1.0f;
}

extern "C" int ccm_sim3_solver_iterate(ccm_sim3_solver* s, int k, int n_iterations, int32_t* found, int32_t* no_more, uint8_t* inliers,
                                       int32_t* n_inliers, float* T12)
{
    if (!s || k < 0 || k >= (int)s->k.size() || !found || !no_more || !n_inliers) return CCM_E_ARG;
    S3rHost& K = s->k[k];
    *found = 0; *no_more = 0; *n_inliers = 0;                               // :122-124
    if (inliers && K.n1 > 0) std::memset(inliers, 0, (size_t)K.n1);
    if (K.n < s->min_inliers || K.n_hyp == 0) { *no_more = 1; return CCM_OK; }          // :129-133 (and N < 3)
    int current = 0;
    while (K.iterations < K.max_its && current < n_iterations) {            // :141
        current++;
        const int h = K.iterations++;
        const int cnt = s->count[(size_t)K.hyp_first + h];
        if (cnt >= K.best_inliers) {                                        // :167
            K.best = h; K.best_inliers = cnt;
            if (cnt > s->min_inliers) {                                     // :176, strict
                *found = 1; *n_inliers = cnt;
                if (inliers) {
                    const uint64_t* m = s->mask.data() + K.mask_first + (size_t)h * K.words;
                    for (int i = 0; i < K.n; i++) if (m[i >> 6] >> (i & 63) & 1) inliers[s->indices1[K.first + i]] = 1;      // :179-181
                }
                if (T12) t12_of(s->rts.data() + 13 * ((size_t)K.hyp_first + h), T12);
                return CCM_OK;
            }
        }
    }
    if (K.iterations >= K.max_its) *no_more = 1;                            // :187
    return CCM_OK;
}

extern "C" int ccm_sim3_solver_find(ccm_sim3_solver* s, int k, int32_t* found, uint8_t* inliers, int32_t* n_inliers, float* T12)
{
    if (!s || k < 0 || k >= (int)s->k.size()) return CCM_E_ARG;
    int32_t flag = 0;
    return ccm_sim3_solver_iterate(s, k, s->k[k].max_its, found, &flag, inliers, n_inliers, T12);
}

extern "C" int ccm_sim3_solver_estimate(const ccm_sim3_solver* s, int k, float* R, float* t, float* scale)
{
    if (!s || k < 0 || k >= (int)s->k.size()) return CCM_E_ARG;
    const S3rHost& K = s->k[k];
    if (K.best < 0) return CCM_E_STATE;
    const float* r = s->rts.data() + 13 * ((size_t)K.hyp_first + K.best);
    if (R) std::memcpy(R, r, 36);
    if (t) std::memcpy(t, r + 9, 12);
    if (scale) *scale = r[12];
    return CCM_OK;
}

extern "C" int ccm_sim3_solver_state(const ccm_sim3_solver* s, int k, int32_t* iterations, int32_t* best_inliers, int32_t* best_hypothesis,
                                     int32_t* max_iterations)
{
    if (!s || k < 0 || k >= (int)s->k.size()) return CCM_E_ARG;
    const S3rHost& K = s->k[k];
    if (iterations) *iterations = K.iterations;
    if (best_inliers) *best_inliers = K.best_inliers;
    if (best_hypothesis) *best_hypothesis = K.best;
    if (max_iterations) *max_iterations = K.max_its;
    return CCM_OK;
}

extern "C" int ccm_sim3_solver_hypotheses(const ccm_sim3_solver* s, int k, int32_t* sample, int32_t* count, float* rts, uint64_t* mask)
{
    if (!s || k < 0 || k >= (int)s->k.size()) return CCM_E_ARG;
    const S3rHost& K = s->k[k];
    const size_t h0 = (size_t)K.hyp_first, H = (size_t)K.n_hyp;
    if (H == 0) return 0;
    if (sample) std::memcpy(sample, s->sample.data() + 3 * h0, H * 12);
    if (count) std::memcpy(count, s->count.data() + h0, H * 4);
    if (rts) std::memcpy(rts, s->rts.data() + 13 * h0, H * 52);
    if (mask) std::memcpy(mask, s->mask.data() + K.mask_first, H * K.words * 8);
    return K.n_hyp;
}
