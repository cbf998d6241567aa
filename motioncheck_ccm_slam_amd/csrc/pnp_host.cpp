// pnp_host.cpp -- C ABI of the batched PnPsolver (src/PnPSolver.cpp): create evaluates every minimal-set hypothesis of every solver in
// one launch and every reachable Refine() in a second one (pnp_kernels.hip); iterate / find replay the ordered bookkeeping of
// PnPsolver::iterate (:155-249) over the stored results on the host.
//
// Which Refine() calls are reachable: Refine (:251-296) runs EPnP over mvbBestInliers, which changes only when a hypothesis becomes
// the running best -- a "record": count >= minInliers and count > every earlier count that reached minInliers.  mnBestInliers starts
// at 0 (carrying it over a later SetRansacParameters is not supported), so the records are a function of the counts alone, whatever
// the calling pattern, and one refinement per record suffices: repeating Refine on the same best is deterministic.  The records are
// found by a scan over the counts on the host after the first download: the counts are needed on the host anyway, the scan is a
// few hundred comparisons per solver, and a device scan would save neither of the two synchronisations (the mask and pose of the
// hypotheses come down with the counts).
#include "mpt_internal.h"
#include "pnp_types.h"
#include "pnp_math.h"
#include <cmath>
#include <memory>

struct PnpState { Staging stage{ false }; };
void pnp_state_free(PnpState* s)
{
    if (!s) return;
    s->stage.release();
    delete s;
}

struct PnpHost {                  // one PnPsolver
    int n = 0, n1 = 0;            // N, mvpMapPointMatches.size()
    int hyp_first = 0, n_hyp = 0, words = 0;
    size_t first = 0, mask_first = 0;
    int ref_first = 0, n_ref = 0; // rows of the refinement outputs
    size_t ref_mask_first = 0;
    int min_inliers = 0;          // mRansacMinInliers after SetRansacParameters
    int max_its = 1;              // mRansacMaxIts
    int iterations = 0;           // mnIterations
    int best_inliers = 0;         // mnBestInliers
    int best = -1;                // hypothesis behind mBestTcw / mvbBestInliers, -1 = none yet
    int best_ref = -1;            // its record (row ref_first + best_ref)
};
struct ccm_pnp_solver {
    int min_set = 4;
    bool detail = false;
    std::vector<PnpHost> k;
    std::vector<int32_t> kp_index, count, sample, ref_hyp, ref_count;
    std::vector<double> rt, ref_rt, det, ref_det;
    std::vector<uint64_t> mask, ref_mask;
};

extern "C" int ccm_pnp_ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                                         int32_t* min_inliers_out, int32_t* max_its_out, float* epsilon_out)
{
    if (n < 0) return CCM_E_ARG;
    int nMinInliers = (int)(n * epsilon);                                   // :124, the product in float
    if (nMinInliers < min_inliers) nMinInliers = min_inliers;
    if (nMinInliers < min_set) nMinInliers = min_set;
    float eps = epsilon;
    const float ratio = n > 0 ? (float)nMinInliers / n : (nMinInliers > 0 ? INFINITY : NAN);      // :131 (IEEE for N = 0)
    if (eps < ratio) eps = ratio;
    int it = 1;                                                             // N < minInliers: undefined in the reference, unused (:163)
    if (n >= nMinInliers && nMinInliers != n) {                             // :137-140
        const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)eps, 3)));
        it = v >= (double)max_iterations ? max_iterations : (v >= 1 ? (int)v : 1);      // the conversion stays inside int's range
    }
    it = std::max(1, std::min(it, max_iterations));                         // :142
    if (min_inliers_out) *min_inliers_out = nMinInliers;
    if (max_its_out) *max_its_out = it;
    if (epsilon_out) *epsilon_out = eps;
    return CCM_OK;
}

namespace {
struct ViewFloat {
    const float* P3D; const float* P2D;
    void get(int i, double pw[3], double uv[2]) const
    {
        pw[0] = P3D[3 * i]; pw[1] = P3D[3 * i + 1]; pw[2] = P3D[3 * i + 2]; uv[0] = P2D[2 * i]; uv[1] = P2D[2 * i + 1];
    }
};
}

extern "C" int ccm_pnp_compute_pose(int n, const float* P3Dw, const float* P2D, const float* K, double* Rt, double* detail)
{
    return ccm_guard(nullptr, "ccm_pnp_compute_pose", [&]() -> int {
        if (n < 4 || !P3Dw || !P2D || !K || !Rt) return CCM_E_ARG;
        const double Kd[4] = { K[0], K[1], K[2], K[3] };
        std::unique_ptr<PnpMatHost> A(new PnpMatHost()), V(new PnpMatHost());
        double out[12];
        pnp_compute_pose(ViewFloat{ P3Dw, P2D }, n, Kd, *A, *V, out, detail);
        std::memcpy(Rt, out, sizeof out);
        return CCM_OK;
    });
}

// Where the correspondences of ccm_pnp_solver_create_frames come from: feature / slot [first[n_solvers]] name a feature of `cur` and a
// slot of `t`; k_pnp_gather fills the P2D / P3D / max_err segments from them.  pb then carries no P2D / P3Dw / sigma2, and kp_index =
// feature.
struct PnpFrames { const ccm_frame* cur; const ccm_map_table* t; const int32_t* feature; const int32_t* slot; const float* level_sigma2; int n_levels; };

// The body of both create calls (fr == nullptr: the correspondences are the caller's arrays), under the caller's ccm_guard.
static int pnp_create(ccm_ctx* c, const ccm_pnp_ransac_problem* pb, const PnpFrames* fr, ccm_pnp_solver** out)
{
    if (!pb || !out || pb->n_solvers < 0) return ccm_fail(c, CCM_E_ARG, "bad PnP RANSAC problem");
    if (pb->min_set < 4 || pb->min_set > PNP_MAXSET) return ccm_fail(c, CCM_E_ARG, "min_set = %d outside [4, %d]", pb->min_set, PNP_MAXSET);
    if (pb->max_iterations < 1 || pb->min_inliers < 0 || pb->reserve < 0)
        return ccm_fail(c, CCM_E_ARG, "bad RANSAC parameters: max_iterations %d, min_inliers %d, reserve %d", pb->max_iterations, pb->min_inliers, pb->reserve);
    const int F = pb->n_solvers, ms = pb->min_set;
    std::unique_ptr<ccm_pnp_solver> S(new ccm_pnp_solver());
    S->min_set = ms; S->detail = (pb->flags & 1u) != 0;
    if (F == 0) { *out = S.release(); return CCM_OK; }
    if (!pb->first || !pb->n1 || !pb->K) return ccm_fail(c, CCM_E_ARG, "bad PnP RANSAC problem: null per-solver array");
    if (pb->first[0] != 0) return ccm_fail(c, CCM_E_ARG, "first[0] must be 0");
    for (int f = 0; f < F; f++) if (pb->first[f + 1] < pb->first[f]) return ccm_fail(c, CCM_E_ARG, "first[] must be non-decreasing");
    const size_t T = (size_t)pb->first[F];
    if (T > 0 && (!pb->kp_index || (fr ? !fr->slot : (!pb->P2D || !pb->P3Dw || !pb->sigma2))))
        return ccm_fail(c, CCM_E_ARG, "bad PnP RANSAC problem: null correspondence array");
    if (fr)
        for (size_t e = 0; e < T; e++)
            if (fr->slot[e] < 0 || fr->slot[e] >= fr->t->capacity)
                return ccm_fail(c, CCM_E_ARG, "correspondence %zu: slot %d outside [0, %d)", e, fr->slot[e], fr->t->capacity);

    // ---- per-solver geometry of the batch, and the checks that keep every index the kernels and iterate() form in range
    S->k.resize(F);
    const size_t rows = (size_t)pb->max_iterations + (size_t)pb->reserve;       // rows of draws per solver
    size_t H = 0, W = 0, n_blocks = 0, Rmax = 0, RWmax = 0;
    for (int f = 0; f < F; f++) {
        PnpHost& k = S->k[f];
        k.first = (size_t)pb->first[f]; k.n = pb->first[f + 1] - pb->first[f]; k.n1 = pb->n1[f];
        if (k.n1 < 0) return ccm_fail(c, CCM_E_ARG, "solver %d: n1 = %d", f, k.n1);
        for (int i = 0; i < k.n; i++) {
            const int32_t kp = pb->kp_index[k.first + i];
            if (kp < 0 || kp >= k.n1) return ccm_fail(c, CCM_E_ARG, "solver %d: kp_index[%d] = %d outside [0, %d)", f, i, kp, k.n1);
        }
        int32_t mi = 0, it = 1;
        ccm_pnp_ransac_parameters(k.n, pb->probability, pb->min_inliers, pb->max_iterations, ms, pb->epsilon, &mi, &it, nullptr);
        k.min_inliers = mi; k.max_its = it;
        k.n_hyp = k.n >= k.min_inliers ? (int)std::min<size_t>((size_t)k.max_its + pb->reserve, (size_t)INT32_MAX / 64) : 0;
        k.words = (k.n + 63) / 64;
        k.hyp_first = (int)H; k.mask_first = W;
        H += (size_t)k.n_hyp; W += (size_t)k.n_hyp * k.words;
        n_blocks += ((size_t)k.n_hyp + PNP_HPB - 1) / PNP_HPB;
        // records have strictly increasing counts in [min_inliers, N]
        const size_t rmax = k.n_hyp ? std::min<size_t>((size_t)k.n_hyp, (size_t)(k.n - k.min_inliers + 1)) : 0;
        Rmax += rmax; RWmax += rmax * k.words;
        if (H > (size_t)INT32_MAX / 256) return ccm_fail(c, CCM_E_ARG, "too many hypotheses in one batch");
    }
    if (H > 0 && !pb->draws) return ccm_fail(c, CCM_E_ARG, "bad PnP RANSAC problem: null draws");
    S->sample.assign(H * (size_t)ms, 0);
    for (int f = 0; f < F; f++) {
        const PnpHost& k = S->k[f];
        const int32_t* d = pb->draws + (size_t)f * rows * ms;
        for (int h = 0; h < k.n_hyp; h++) {
            for (int i = 0; i < ms; i++)
                if (d[ms * h + i] < 0 || d[ms * h + i] > k.n - 1 - i)
                    return ccm_fail(c, CCM_E_ARG, "solver %d, hypothesis %d: draw %d = %d outside [0, %d]", f, h, i, d[ms * h + i], k.n - 1 - i);
            pnp_sample(k.n, ms, d + (size_t)ms * h, S->sample.data() + ((size_t)k.hyp_first + h) * ms);       // :178-192
        }
    }
    S->kp_index.assign(pb->kp_index, pb->kp_index + T);
    if (H == 0) { *out = S.release(); return CCM_OK; }                  // nothing to evaluate: every solver reports bNoMore

    // ---- staging: [solvers | blocks | sample | P2D | P3D | max_err] up, [status | count | Rt | mask | detail] down, then [records]
    // up and [count | Rt | mask | detail] of the refinements down.  With frames [feature | slot | level_sigma2] go up in the place
    // of P2D | P3D | max_err, which k_pnp_gather fills on the device.
    const size_t DB = S->detail ? (size_t)PNP_DETAIL * 8 : 0;
    size_t off = 0;
    const size_t o_solvers = seg(off, (size_t)F * sizeof(PnpSolver)), o_blocks = seg(off, n_blocks * sizeof(PnpBlock));
    const size_t o_sample = seg(off, H * PNP_MAXSET * 4);
    const size_t o_feat = seg(off, fr ? T * 4 : 0), o_slot = seg(off, fr ? T * 4 : 0), o_sig = seg(off, fr ? CCM_MAX_LEVELS * 4 : 0);
    const size_t up_end = off;                                          // with frames: the end of the upload
    const size_t o_p2 = seg(off, T * 8), o_p3 = seg(off, T * 12), o_me = seg(off, T * 4);
    const size_t in_end = off;
    const size_t o_status = seg(off, 16);
    const size_t o_count = seg(off, H * 4), o_rt = seg(off, H * 96), o_mask = seg(off, W * 8), o_det = seg(off, H * DB);
    const size_t out_end = off;
    const size_t o_rec = seg(off, Rmax * sizeof(PnpRecord));
    const size_t rec_end = off;
    const size_t o_rcount = seg(off, Rmax * 4), o_rrt = seg(off, Rmax * 96), o_rmask = seg(off, RWmax * 8), o_rdet = seg(off, Rmax * DB);
    const size_t end = off;
    CCM_HIP(c, hipSetDevice(c->device));
    if (!c->pnp) c->pnp = new PnpState();
    Staging& G = c->pnp->stage;
    int rc;
    if ((rc = G.reserve(c, end))) return rc;
    PnpSolver* hs = G.host<PnpSolver>(o_solvers);
    PnpBlock* hb = G.host<PnpBlock>(o_blocks);
    int32_t* hsm = G.host<int32_t>(o_sample);
    size_t nb = 0;
    for (int f = 0; f < F; f++) {
        const PnpHost& k = S->k[f];
        PnpSolver& s = hs[f];
        std::memset(&s, 0, sizeof s);
        s.first = (int32_t)k.first; s.n = k.n; s.hyp_first = k.hyp_first; s.n_hyp = k.n_hyp; s.words = k.words; s.min_set = ms;
        s.mask_first = (int64_t)k.mask_first;
        std::memcpy(s.K, pb->K + 4 * f, 16);
        for (int h0 = 0; h0 < k.n_hyp; h0 += PNP_HPB) hb[nb++] = PnpBlock{ f, h0, std::min(PNP_HPB, k.n_hyp - h0), 0 };
        for (int h = 0; h < k.n_hyp; h++)
            for (int i = 0; i < PNP_MAXSET; i++)
                hsm[((size_t)k.hyp_first + h) * PNP_MAXSET + i] = i < ms ? S->sample[((size_t)k.hyp_first + h) * ms + i] : 0;
    }
    const PnpDev D{ G.dev<PnpSolver>(o_solvers), G.dev<PnpBlock>(o_blocks), G.dev<float>(o_p2), G.dev<float>(o_p3), G.dev<float>(o_me),
                    G.dev<int32_t>(o_sample), G.dev<int32_t>(o_count), G.dev<double>(o_rt), G.dev<unsigned long long>(o_mask),
                    S->detail ? G.dev<double>(o_det) : nullptr };
    if (fr) {
        G.put(o_feat, fr->feature, T * 4); G.put(o_slot, fr->slot, T * 4);
        fill_levels(G.host<float>(o_sig), fr->level_sigma2, fr->n_levels);
        if ((rc = G.upload(c, 0, up_end))) return rc;
        CCM_HIP(c, hipMemsetAsync(G.dev<int32_t>(o_status), 0, 16, c->stream));
        const MptTable& Tb = fr->t->T;
        pnp_gather_launch(c->stream, PnpGather{ (int32_t)T, fr->cur->n, Tb.capacity, fr->n_levels, pb->th2, G.dev<int32_t>(o_feat), G.dev<int32_t>(o_slot),
                                                fr->cur->kx, fr->cur->ky, fr->cur->oct, Tb.pos, Tb.flags, G.dev<float>(o_sig),
                                                G.dev<float>(o_p2), G.dev<float>(o_p3), G.dev<float>(o_me), G.dev<int32_t>(o_status) });
        CCM_HIP(c, hipGetLastError());
    } else {
        float* hme = G.host<float>(o_me);
        for (size_t e = 0; e < T; e++) hme[e] = pb->sigma2[e] * pb->th2;    // mvMaxError (:146), a float product
        G.put(o_p2, pb->P2D, T * 8); G.put(o_p3, pb->P3Dw, T * 12);
        if ((rc = G.upload(c, 0, in_end))) return rc;
    }
    pnp_hypotheses_launch(c->stream, D, (int)n_blocks);
    CCM_HIP(c, hipGetLastError());
    if ((rc = G.download(c, fr ? o_status : o_count, out_end)) || (rc = G.wait(c))) return rc;
    if (fr && *G.host<int32_t>(o_status))
        return ccm_fail(c, CCM_E_ARG, "a correspondence names a feature outside [0, %d), a slot that is not LIVE or an octave outside [0, %d)",
                        fr->cur->n, fr->n_levels);
    {
        const int32_t* rn = G.host<int32_t>(o_count); const double* rr = G.host<double>(o_rt);
        const uint64_t* rm = G.host<uint64_t>(o_mask); const double* rd = G.host<double>(o_det);
        S->count.assign(rn, rn + H); S->rt.assign(rr, rr + 12 * H); S->mask.assign(rm, rm + W);
        if (S->detail) S->det.assign(rd, rd + PNP_DETAIL * H);
    }

    // ---- the records (see the head of this file), one Refine() each
    PnpRecord* hr = G.host<PnpRecord>(o_rec);
    size_t R = 0, RW = 0;
    for (int f = 0; f < F; f++) {
        PnpHost& k = S->k[f];
        k.ref_first = (int)R; k.ref_mask_first = RW;
        int best = 0;
        for (int h = 0; h < k.n_hyp; h++) {
            const int cnt = S->count[(size_t)k.hyp_first + h];
            if (cnt >= k.min_inliers && cnt > best && cnt <= k.n && R < Rmax && RW + k.words <= RWmax) {      // :200-206
                best = cnt;
                hr[R] = PnpRecord{ f, h, (int32_t)R, 0, (int64_t)RW };
                S->ref_hyp.push_back(h);
                R++; RW += (size_t)k.words; k.n_ref++;
            }
        }
    }
    if (R > 0) {
        if ((rc = G.upload(c, o_rec, o_rec + R * sizeof(PnpRecord)))) return rc;
        const PnpRefineDev Q{ D.solvers, G.dev<PnpRecord>(o_rec), D.P2D, D.P3D, D.max_err, D.mask, G.dev<int32_t>(o_rcount),
                              G.dev<double>(o_rrt), G.dev<unsigned long long>(o_rmask), S->detail ? G.dev<double>(o_rdet) : nullptr };
        pnp_refine_launch(c->stream, Q, (int)R);
        CCM_HIP(c, hipGetLastError());
        if ((rc = G.download(c, rec_end, end)) || (rc = G.wait(c))) return rc;
        const int32_t* rn = G.host<int32_t>(o_rcount); const double* rr = G.host<double>(o_rrt);
        const uint64_t* rm = G.host<uint64_t>(o_rmask); const double* rd = G.host<double>(o_rdet);
        S->ref_count.assign(rn, rn + R); S->ref_rt.assign(rr, rr + 12 * R); S->ref_mask.assign(rm, rm + RW);
        if (S->detail) S->ref_det.assign(rd, rd + PNP_DETAIL * R);
    }
    *out = S.release();
    return CCM_OK;
}

extern "C" int ccm_pnp_solver_create(ccm_ctx* c, const ccm_pnp_ransac_problem* pb, ccm_pnp_solver** out)
{
    RoctxRange roctx_("ccm_pnp_solver_create");
    return ccm_guard(c, "ccm_pnp_solver_create", [&]() -> int {
        if (!c) return CCM_E_ARG;
        return pnp_create(c, pb, nullptr, out);
    });
}

extern "C" int ccm_pnp_solver_create_frames(ccm_ctx* c, ccm_frame* cur, ccm_map_table* t, const ccm_pnp_frames_problem* fp, ccm_pnp_solver** out)
{
    RoctxRange roctx_("ccm_pnp_solver_create_frames");
    if (!c || !cur || !t || !fp || !out) return CCM_E_ARG;
    const char* fn = "ccm_pnp_solver_create_frames";
    int rc;
    if ((rc = frame_named_check(c, cur, CCM_E_STATE, fn, "cur")) || (rc = check_table(c, t))) return rc;
    if (fp->n_solvers < 0 || fp->n_levels < 1 || fp->n_levels > CCM_MAX_LEVELS || !fp->level_sigma2)
        return ccm_fail(c, CCM_E_ARG, "%s: n_solvers = %d, n_levels = %d (1..%d), level_sigma2 %s", fn, fp->n_solvers, fp->n_levels, CCM_MAX_LEVELS,
                        fp->level_sigma2 ? "given" : "null");
    if (fp->n_solvers > 0 && !fp->first) return ccm_fail(c, CCM_E_ARG, "%s: null first", fn);
    const int T = fp->n_solvers > 0 ? fp->first[fp->n_solvers] : 0;
    if (T > 0 && (!fp->feature || !fp->slot)) return ccm_fail(c, CCM_E_ARG, "%s: null correspondence array", fn);
    return table_call(c, t, false, fn, [&]() -> int {                       // reads pos and flags
        const std::vector<int32_t> n1((size_t)std::max(fp->n_solvers, 1), cur->n);      // mvpMapPointMatches.size() = the frame's N
        const ccm_pnp_ransac_problem pb{ fp->n_solvers, fp->first, n1.data(), fp->K, nullptr, nullptr, nullptr, fp->feature, fp->probability,
                                         fp->min_inliers, fp->max_iterations, fp->min_set, fp->epsilon, fp->th2, fp->reserve, fp->draws, fp->flags };
        const PnpFrames fr{ cur, t, fp->feature, fp->slot, fp->level_sigma2, fp->n_levels };
        return pnp_create(c, &pb, &fr, out);
    });
}

extern "C" void ccm_pnp_solver_destroy(ccm_pnp_solver* s) { delete s; }

extern "C" int ccm_pnp_solver_count(const ccm_pnp_solver* s) { return s ? (int)s->k.size() : CCM_E_ARG; }

// [R | t; 0 0 0 1] converted to float (:208-214, :285-291)
static void tcw_of(const double* rt, float* Tcw)
{
    for (int r = 0; r < 3; r++) {
        for (int col = 0; col < 3; col++) Tcw[4 * r + col] = (float)rt[3 * r + col];
        Tcw[4 * r + 3] = (float)rt[9 + r];
    }
    Tcw[12] = Tcw[13] = Tcw[14] = 0.0f; Tcw[15] = 1.0f;
}
static void scatter(const ccm_pnp_solver* s, const PnpHost& K, const uint64_t* m, uint8_t* inliers)
{
    if (!inliers) return;
    for (int i = 0; i < K.n; i++) if (m[i >> 6] >> (i & 63) & 1) inliers[s->kp_index[K.first + i]] = 1;
}

static int pnp_iterate(ccm_pnp_solver* s, int k, int n_iterations, int32_t* found, int32_t* no_more, uint8_t* inliers, int32_t* n_inliers,
                       float* Tcw)
{
    PnpHost& K = s->k[k];
    const int64_t ask = std::max<int64_t>(n_iterations, 0);
    if (K.n >= K.min_inliers && std::max<int64_t>(K.max_its, (int64_t)K.iterations + ask) > K.n_hyp) return CCM_E_STATE;     // beyond the reserve
    *found = 0; *n_inliers = 0;                                             // :157-159
    if (no_more) *no_more = 0;
    if (inliers && K.n1 > 0) std::memset(inliers, 0, (size_t)K.n1);
    if (K.n < K.min_inliers) { if (no_more) *no_more = 1; return CCM_OK; }  // :163-167
    int current = 0;
    while (K.iterations < K.max_its || current < n_iterations) {            // :172, with its ||
        current++;
        const int h = K.iterations++;
        const int cnt = s->count[(size_t)K.hyp_first + h];
        if (cnt >= K.min_inliers) {                                         // :200
            if (cnt > K.best_inliers) { K.best = h; K.best_inliers = cnt; K.best_ref++; }     // :203-215; the records in their order
            const size_t r = (size_t)K.ref_first + K.best_ref;              // Refine() of the current best (:217)
            if (s->ref_count[r] > K.min_inliers) {                          // :283, strict
                *found = 1; *n_inliers = s->ref_count[r];
                scatter(s, K, s->ref_mask.data() + K.ref_mask_first + (size_t)K.best_ref * K.words, inliers);        // :221-225
                if (Tcw) tcw_of(s->ref_rt.data() + 12 * r, Tcw);
                return CCM_OK;
            }
        }
    }
    if (K.iterations >= K.max_its) {                                        // :232-246
        if (no_more) *no_more = 1;
        if (K.best_inliers >= K.min_inliers) {
            *found = 1; *n_inliers = K.best_inliers;
            scatter(s, K, s->mask.data() + K.mask_first + (size_t)K.best * K.words, inliers);
            if (Tcw) tcw_of(s->rt.data() + 12 * ((size_t)K.hyp_first + K.best), Tcw);
        }
    }
    return CCM_OK;
}

extern "C" int ccm_pnp_solver_iterate(ccm_pnp_solver* s, int k, int n_iterations, int32_t* found, int32_t* no_more, uint8_t* inliers,
                                      int32_t* n_inliers, float* Tcw)
{
    if (!s || k < 0 || k >= (int)s->k.size() || !found || !no_more || !n_inliers) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_pnp_solver_iterate", [&]() -> int { return pnp_iterate(s, k, n_iterations, found, no_more, inliers, n_inliers, Tcw); });
}

extern "C" int ccm_pnp_solver_find(ccm_pnp_solver* s, int k, int32_t* found, uint8_t* inliers, int32_t* n_inliers, float* Tcw)
{
    if (!s || k < 0 || k >= (int)s->k.size() || !found || !n_inliers) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_pnp_solver_find", [&]() -> int { return pnp_iterate(s, k, s->k[k].max_its, found, nullptr, inliers, n_inliers, Tcw); });
}

extern "C" int ccm_pnp_solver_state(const ccm_pnp_solver* s, int k, int32_t* iterations, int32_t* best_inliers, int32_t* best_hypothesis,
                                    int32_t* max_iterations, int32_t* min_inliers)
{
    if (!s || k < 0 || k >= (int)s->k.size()) return CCM_E_ARG;
    const PnpHost& K = s->k[k];
    if (iterations) *iterations = K.iterations;
    if (best_inliers) *best_inliers = K.best_inliers;
    if (best_hypothesis) *best_hypothesis = K.best;
    if (max_iterations) *max_iterations = K.max_its;
    if (min_inliers) *min_inliers = K.min_inliers;
    return CCM_OK;
}

extern "C" int ccm_pnp_solver_hypotheses(const ccm_pnp_solver* s, int k, int32_t* sample, int32_t* count, double* Rt, uint64_t* mask, double* detail)
{
    if (!s || k < 0 || k >= (int)s->k.size()) return CCM_E_ARG;
    if (detail && !s->detail) return CCM_E_STATE;
    const PnpHost& K = s->k[k];
    const size_t h0 = (size_t)K.hyp_first, H = (size_t)K.n_hyp;
    if (H == 0) return 0;
    if (sample) std::memcpy(sample, s->sample.data() + s->min_set * h0, H * s->min_set * 4);
    if (count) std::memcpy(count, s->count.data() + h0, H * 4);
    if (Rt) std::memcpy(Rt, s->rt.data() + 12 * h0, H * 96);
    if (mask) std::memcpy(mask, s->mask.data() + K.mask_first, H * K.words * 8);
    if (detail) std::memcpy(detail, s->det.data() + PNP_DETAIL * h0, H * PNP_DETAIL * 8);
    return K.n_hyp;
}

extern "C" int ccm_pnp_solver_refinements(const ccm_pnp_solver* s, int k, int32_t* hyp, int32_t* count, double* Rt, uint64_t* mask, double* detail)
{
    if (!s || k < 0 || k >= (int)s->k.size()) return CCM_E_ARG;
    if (detail && !s->detail) return CCM_E_STATE;
    const PnpHost& K = s->k[k];
    const size_t r0 = (size_t)K.ref_first, R = (size_t)K.n_ref;
    if (R == 0) return 0;
    if (hyp) std::memcpy(hyp, s->ref_hyp.data() + r0, R * 4);
    if (count) std::memcpy(count, s->ref_count.data() + r0, R * 4);
    if (Rt) std::memcpy(Rt, s->ref_rt.data() + 12 * r0, R * 96);
    if (mask) std::memcpy(mask, s->ref_mask.data() + K.ref_mask_first, R * K.words * 8);
    if (detail) std::memcpy(detail, s->ref_det.data() + PNP_DETAIL * r0, R * PNP_DETAIL * 8);
    return K.n_ref;
}
