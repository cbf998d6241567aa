// init_host.cpp -- C ABI of the monocular Initializer (src/Initializer.cpp).  ccm_initialize gathers the matches, runs Normalize and the
// sampling of :78-93 on the host, evaluates every hypothesis in one launch (k_init_hypotheses), replays the ordered selection of
// :144-167 / :195-218 over the stored scores, decomposes the chosen model into its 8 (ReconstructH) or 4 (ReconstructF) motion
// hypotheses on the host, tests all of them in one launch (k_init_check_rt) and replays the decisions of :495-565 / :685-727.
#include "staging.h"
#include "init_types.h"
#include "init_math.h"
#include <cmath>

// The staging area (staging.h), laid out [inputs | hypothesis outputs | CheckRT outputs].
struct InitState { Staging stage{ false }; };
void init_state_free(InitState* s)
{
    if (!s) return;
    s->stage.release();
    delete s;
}

// Normalize (:745-791) without the point list: sX, sY, meanX, meanY.  Float sums in index order over all keypoints.
static void normalize(const float* xy, int n, float out[4])
{
    float meanX = 0, meanY = 0;
    for (int i = 0; i < n; i++) { meanX += xy[2 * i]; meanY += xy[2 * i + 1]; }
    meanX = meanX / n; meanY = meanY / n;
    float meanDevX = 0, meanDevY = 0;
    for (int i = 0; i < n; i++) { meanDevX += std::fabs(xy[2 * i] - meanX); meanDevY += std::fabs(xy[2 * i + 1] - meanY); }
    meanDevX = meanDevX / n; meanDevY = meanDevY / n;
    out[0] = 1.0f / meanDevX; out[1] = 1.0f / meanDevY; out[2] = meanX; out[3] = meanY;
}

// A = U diag(w) Vt with w descending, from a Jacobi in double on A^T A; stored as float like the reference's CV_32F results.
// The left vectors are A v / w.  The third one is u1 x u2 instead when cross_u3 is set (a rank-2 matrix: DecomposeE) or when w3 is not
// positive (a rank-deficient H): the completion of the basis an SVD would return, up to its sign.  A matrix of rank < 2 leaves a zero
// column (w1 or w2 = 0); ReconstructH's ratios are then inf / NaN, nothing exits at :593 and no candidate collects a good point.
static void svd3(const float* A, float* U, float* w, float* Vt, bool cross_u3)
{
    double B[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) B[i][j] = (double)A[i] * A[j] + (double)A[3 + i] * A[3 + j] + (double)A[6 + i] * A[6 + j];
    ini_jacobi<3>(B, V);
    int o[3] = { 0, 1, 2 };
    std::sort(o, o + 3, [&](int a, int b) { return B[a][a] > B[b][b]; });
    double u[3][3] = { { 0 } };                                             // u[j] = j-th left vector
    for (int j = 0; j < 3; j++) {
        const double sv = std::sqrt(std::max(B[o[j]][o[j]], 0.0));
        w[j] = (float)sv;
        for (int k = 0; k < 3; k++) Vt[3 * j + k] = (float)V[k][o[j]];
        if (j == 2 && (cross_u3 || !(sv > 0.0))) {
            u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1]; u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2]; u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
        } else if (sv > 0.0) {
            for (int r = 0; r < 3; r++) u[j][r] = ((double)A[3 * r] * V[0][o[j]] + (double)A[3 * r + 1] * V[1][o[j]] + (double)A[3 * r + 2] * V[2][o[j]]) / sv;
        }
    }
    for (int j = 0; j < 3; j++)
        for (int r = 0; r < 3; r++) U[3 * r + j] = (float)u[j][r];
}
static double det3(const float* A)
{
    return (double)A[0] * ((double)A[4] * A[8] - (double)A[5] * A[7]) - (double)A[1] * ((double)A[3] * A[8] - (double)A[5] * A[6])
         + (double)A[2] * ((double)A[3] * A[7] - (double)A[4] * A[6]);
}
static void transpose3(const float* A, float* B) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) B[3 * r + c] = A[3 * c + r]; }
static void mulv3(const float* A, const float* x, float* y)
{
    for (int r = 0; r < 3; r++) y[r] = (float)((double)A[3 * r] * x[0] + (double)A[3 * r + 1] * x[1] + (double)A[3 * r + 2] * x[2]);
}
static void unit3(float* t)
{
    const double n = std::sqrt((double)t[0] * t[0] + (double)t[1] * t[1] + (double)t[2] * t[2]);
    for (int k = 0; k < 3; k++) t[k] = (float)(t[k] / n);
}
static void finish_candidate(const float K[4], IniCand& c)
{
    float Rt[9]; transpose3(c.R, Rt);
    mulv3(Rt, c.t, c.O2);                                                   // O2 = -R^T t (:822)
    for (int k = 0; k < 3; k++) c.O2[k] = -c.O2[k];
    const float Km[9] = { K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1 };          // P2 = K [R | t] (:817-820)
    for (int r = 0; r < 3; r++)
        for (int col = 0; col < 4; col++) {
            double a = 0;
            for (int k = 0; k < 3; k++) a += (double)Km[3 * r + k] * (col < 3 ? c.R[3 * k + col] : c.t[k]);
            c.P2[4 * r + col] = (float)a;
        }
}

// The four motion hypotheses of ReconstructF (:474-493) in the order of the CheckRT calls: (R1, t), (R2, t), (R1, -t), (R2, -t)
static int candidates_f(const float* F21, const float K[4], IniCand* c)
{
    const float Km[9] = { K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1 };
    float Kt[9], P[9], E[9], U[9], w[3], Vt[9];
    transpose3(Km, Kt);
    ini_mul3(Kt, F21, P); ini_mul3(P, Km, E);                               // E21 = K^T F21 K (:475)
    svd3(E, U, w, Vt, true);                                                // DecomposeE (:905-925)
    float t[3] = { U[2], U[5], U[8] };
    unit3(t);
    const float W[9] = { 0, -1, 0, 1, 0, 0, 0, 0, 1 };
    float Wt[9], R1[9], R2[9];
    transpose3(W, Wt);
    ini_mul3(U, W, P); ini_mul3(P, Vt, R1);
    if (det3(R1) < 0) for (int k = 0; k < 9; k++) R1[k] = -R1[k];
    ini_mul3(U, Wt, P); ini_mul3(P, Vt, R2);
    if (det3(R2) < 0) for (int k = 0; k < 9; k++) R2[k] = -R2[k];
    for (int i = 0; i < 4; i++) {
        std::memcpy(c[i].R, (i & 1) ? R2 : R1, 36);
        for (int k = 0; k < 3; k++) c[i].t[k] = i < 2 ? t[k] : -t[k];
        finish_candidate(K, c[i]);
    }
    return 4;
}

// The eight motion hypotheses of ReconstructH (:580-682), or 0 for the early exit of :593
static int candidates_h(const float* H21, const float K[4], IniCand* c)
{
    const float Km[9] = { K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1 };
    float invK[9], P[9], A[9], U[9], w[3], Vt[9];
    ini_inv3(Km, invK);
    ini_mul3(invK, H21, P); ini_mul3(P, Km, A);                             // A = invK * H21 * K (:581)
    svd3(A, U, w, Vt, false);
    const float s = (float)(det3(U) * det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return 0;                   // :593
    const float aux1 = std::sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = std::sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[] = { aux1, aux1, -aux1, -aux1 };
    const float x3[] = { aux3, -aux3, aux3, -aux3 };
    const float aux_stheta = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);      // case d' = d2
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[] = { aux_stheta, -aux_stheta, -aux_stheta, aux_stheta };
    const float aux_sphi = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);        // case d' = -d2
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[] = { aux_sphi, -aux_sphi, -aux_sphi, aux_sphi };
    float sU[9];
    for (int k = 0; k < 9; k++) sU[k] = s * U[k];
    for (int i = 0; i < 8; i++) {
        const int j = i & 3;
        float Rp[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, tp[3];
        if (i < 4) {                                                        // :615-644
            Rp[0] = ctheta; Rp[2] = -stheta[j]; Rp[6] = stheta[j]; Rp[8] = ctheta;
            tp[0] = x1[j]; tp[1] = 0; tp[2] = -x3[j];
            for (int k = 0; k < 3; k++) tp[k] *= d1 - d3;
        } else {                                                            // :652-682
            Rp[0] = cphi; Rp[2] = sphi[j]; Rp[4] = -1; Rp[6] = sphi[j]; Rp[8] = -cphi;
            tp[0] = x1[j]; tp[1] = 0; tp[2] = x3[j];
            for (int k = 0; k < 3; k++) tp[k] *= d1 + d3;
        }
        ini_mul3(sU, Rp, P); ini_mul3(P, Vt, c[i].R);                       // R = s * U * Rp * Vt
        mulv3(U, tp, c[i].t);
        unit3(c[i].t);                                                      // t / norm(t)
        finish_candidate(K, c[i]);
    }
    return 8;
}

// :892-900 over the cosParallax values CheckRT pushed, in match order
static float parallax_of(std::vector<float>& cosp)
{
    if (cosp.empty()) return 0.0f;
    std::sort(cosp.begin(), cosp.end());
    const size_t idx = std::min<size_t>(50, cosp.size() - 1);
    return (float)((double)(std::acos(cosp[idx]) * 180.0f) / 3.1415926535897932384626433832795);
}

// The decision of ReconstructF (:495-565) over nGood / parallax of its four candidates, N = the inliers of F: the chosen candidate or -1
static int decide_f(const int32_t* nGood, const float* parallax, int N, float minParallax, int minTriangulated)
{
    const int maxGood = std::max(nGood[0], std::max(nGood[1], std::max(nGood[2], nGood[3])));
    const int nMinGood = std::max(static_cast<int>(0.9 * N), minTriangulated);
    int nsimilar = 0;
    for (int i = 0; i < 4; i++) if (nGood[i] > 0.7 * maxGood) nsimilar++;
    if (maxGood < nMinGood || nsimilar > 1) return -1;
    for (int i = 0; i < 4; i++)
        if (maxGood == nGood[i]) return parallax[i] > minParallax ? i : -1;  // the else-if chain: only the first equal candidate is asked
    return -1;
}
// The decision of ReconstructH (:685-727) over its eight candidates
static int decide_h(const int32_t* nGood, const float* parallax, int N, float minParallax, int minTriangulated)
{
    int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
    float bestParallax = -1;
    for (int i = 0; i < 8; i++) {
        if (nGood[i] > bestGood) { secondBestGood = bestGood; bestGood = nGood[i]; bestSolutionIdx = i; bestParallax = parallax[i]; }
        else if (nGood[i] > secondBestGood) secondBestGood = nGood[i];
    }
    if (secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated && bestGood > 0.9 * N) return bestSolutionIdx;
    return -1;
}

extern "C" int ccm_initialize(ccm_ctx* c, const ccm_initializer_problem* pb, ccm_initializer_result* res)
{
    RoctxRange roctx_("ccm_initialize");
    return ccm_guard(c, "ccm_initialize", [&]() -> int {
        if (!pb || !res) return ccm_fail(c, CCM_E_ARG, "ccm_initialize: null problem or result");
        if (pb->n1 < 0 || pb->n2 < 0) return ccm_fail(c, CCM_E_ARG, "ccm_initialize: n1 = %d, n2 = %d", pb->n1, pb->n2);
        if (pb->n1 > 0 && (!pb->kp1_xy || !pb->matches12)) return ccm_fail(c, CCM_E_ARG, "ccm_initialize: null %s", !pb->kp1_xy ? "kp1_xy" : "matches12");
        if (pb->n2 > 0 && !pb->kp2_xy) return ccm_fail(c, CCM_E_ARG, "ccm_initialize: null kp2_xy");
        if (pb->n1 > 0 && (!res->p3d || !res->triangulated)) return ccm_fail(c, CCM_E_ARG, "ccm_initialize: null %s", !res->p3d ? "p3d" : "triangulated");
        if (pb->max_iterations < 1) return ccm_fail(c, CCM_E_ARG, "ccm_initialize: max_iterations = %d", pb->max_iterations);
        const int iters = pb->max_iterations;
        // mvMatches12 (:47-59)
        std::vector<int32_t> m1, m2;
        for (int i = 0; i < pb->n1; i++) {
            const int32_t j = pb->matches12[i];
            if (j < 0) continue;
            if (j >= pb->n2) return ccm_fail(c, CCM_E_ARG, "ccm_initialize: matches12[%d] = %d outside [0, %d)", i, j, pb->n2);
            m1.push_back(i); m2.push_back(j);
        }
        const int N = (int)m1.size();
        ccm_initializer_tap* tap = res->tap;
        float* const p3d = res->p3d; uint8_t* const tri = res->triangulated;
        auto clear_outputs = [&]() {
            if (pb->n1 > 0) { std::memset(p3d, 0, (size_t)pb->n1 * 12); std::memset(tri, 0, (size_t)pb->n1); }
            res->initialized = 0; res->model = 1; res->score_h = 0; res->score_f = 0; res->best_h = -1; res->best_f = -1; res->n_matches = N;
            if (tap) tap->n_candidates = 0;
        };
        if (N < 8) { clear_outputs(); return CCM_OK; }
        // mvSets (:78-93)
        if (!pb->draws) return ccm_fail(c, CCM_E_ARG, "ccm_initialize: null draws");
        std::vector<int32_t> sets((size_t)iters * 8);
        {
            std::vector<int32_t> avail(N);                                  // vAllIndices (:68-71)
            for (int i = 0; i < N; i++) avail[i] = i;
            for (int it = 0; it < iters; it++) {
                int32_t pos[8], old[8];
                int size = N;
                for (int j = 0; j < 8; j++) {
                    const int32_t r = pb->draws[8 * (size_t)it + j];
                    if (r < 0 || r > size - 1) return ccm_fail(c, CCM_E_ARG, "ccm_initialize: set %d: draw %d = %d outside [0, %d]", it, j, r, size - 1);
                    sets[8 * (size_t)it + j] = avail[r];
                    pos[j] = r; old[j] = avail[r];
                    avail[r] = avail[size - 1];                             // :90-91; the popped tail keeps its values
                    size--;
                }
                for (int k = 7; k >= 0; k--) avail[pos[k]] = old[k];        // vAvailableIndices = vAllIndices (:80)
            }
        }
        if (!c) return CCM_E_ARG;                                           // everything above needs no context
        const float K[4] = { pb->fx, pb->fy, pb->cx, pb->cy };
        float T1[4], T2[4];
        normalize(pb->kp1_xy, pb->n1, T1); normalize(pb->kp2_xy, pb->n2, T2);

        // ---- staging: [m | sets] up, [H21 | H12 | F21 | scores | masks] down, then [flags | cos | X] down
        const size_t words = ((size_t)N + 63) / 64;
        size_t off = 0;
        const size_t o_m = seg(off, (size_t)N * 16), o_sets = seg(off, (size_t)iters * 32);
        const size_t in_end = off;
        const size_t o_h21 = seg(off, (size_t)iters * 36), o_h12 = seg(off, (size_t)iters * 36), o_f21 = seg(off, (size_t)iters * 36);
        const size_t o_sh = seg(off, (size_t)iters * 4), o_sf = seg(off, (size_t)iters * 4);
        const size_t o_mh = seg(off, (size_t)iters * words * 8), o_mf = seg(off, (size_t)iters * words * 8);
        const size_t a_end = off;
        const size_t o_flags = seg(off, (size_t)INI_MAX_CAND * N), o_cos = seg(off, (size_t)INI_MAX_CAND * N * 4), o_x = seg(off, (size_t)INI_MAX_CAND * N * 12);
        const size_t end = off;
        CCM_HIP(c, hipSetDevice(c->device));
        if (!c->init) c->init = new InitState();
        Staging& G = c->init->stage;
        int rc;
        if ((rc = G.reserve(c, end))) return rc;
        float* hm = G.host<float>(o_m);
        for (int i = 0; i < N; i++) {
            hm[4 * i] = pb->kp1_xy[2 * (size_t)m1[i]]; hm[4 * i + 1] = pb->kp1_xy[2 * (size_t)m1[i] + 1];
            hm[4 * i + 2] = pb->kp2_xy[2 * (size_t)m2[i]]; hm[4 * i + 3] = pb->kp2_xy[2 * (size_t)m2[i] + 1];
        }
        G.put(o_sets, sets.data(), sets.size() * 4);
        hipStream_t st = c->stream;
        if ((rc = G.upload(c, 0, in_end))) return rc;
        IniDev D{};
        D.m = G.dev<float>(o_m); D.sets = G.dev<int32_t>(o_sets);
        D.n = N; D.iters = iters; D.words = (int32_t)words;
        std::memcpy(D.T1, T1, 16); std::memcpy(D.T2, T2, 16);
        D.inv_sigma2 = (float)(1.0 / (double)(pb->sigma * pb->sigma));       // :331, :407
        D.H21 = G.dev<float>(o_h21); D.H12 = G.dev<float>(o_h12); D.F21 = G.dev<float>(o_f21);
        D.score_h = G.dev<float>(o_sh); D.score_f = G.dev<float>(o_sf);
        D.mask_h = G.dev<unsigned long long>(o_mh); D.mask_f = G.dev<unsigned long long>(o_mf);
        init_hypotheses_launch(st, D);
        CCM_HIP(c, hipGetLastError());
        if ((rc = G.download(c, in_end, a_end)) || (rc = G.wait(c))) return rc;

        // ---- :144-167 / :195-218: the first strictly greater score wins, starting from 0.0
        const float* sh = G.host<float>(o_sh); const float* sf = G.host<float>(o_sf);
        float SH = 0.0f, SF = 0.0f; int best_h = -1, best_f = -1;
        for (int it = 0; it < iters; it++) {
            if (sh[it] > SH) { SH = sh[it]; best_h = it; }
            if (sf[it] > SF) { SF = sf[it]; best_f = it; }
        }
        const float RH = SH / (SH + SF);                                    // :108
        const int model = RH > 0.40 ? 0 : 1;                                // :111; NaN compares false
        const int best = model == 0 ? best_h : best_f;
        IniRtDev R{};
        int n_cand = 0;
        if (best >= 0)
            n_cand = model == 0 ? candidates_h(G.host<float>(o_h21) + 9 * (size_t)best, K, R.cand)
                                : candidates_f(G.host<float>(o_f21) + 9 * (size_t)best, K, R.cand);
        int32_t nGood[INI_MAX_CAND] = { 0 }; float parallax[INI_MAX_CAND] = { 0 };
        int chosen = -1;
        const uint8_t* flags = G.host<uint8_t>(o_flags); const float* cosv = G.host<float>(o_cos); const float* X = G.host<float>(o_x);
        if (n_cand > 0) {
            R.m = D.m; R.mask = (model == 0 ? D.mask_h : D.mask_f) + (size_t)best * words;
            R.n = N; R.n_cand = n_cand;
            std::memcpy(R.K, K, 16);
            R.th2 = (float)(4.0 * (double)(pb->sigma * pb->sigma));          // 4.0 * mSigma2 (:490)
            R.flags = G.dev<uint8_t>(o_flags); R.cosp = G.dev<float>(o_cos); R.X = G.dev<float>(o_x);
            init_check_rt_launch(st, R);
            CCM_HIP(c, hipGetLastError());
            if ((rc = G.download(c, a_end, end)) || (rc = G.wait(c))) return rc;
            const uint64_t* bm = G.host<uint64_t>(model == 0 ? o_mh : o_mf) + (size_t)best * words;
            int n_in = 0;                                                   // N of :469-472 / :571-574
            for (size_t wd = 0; wd < words; wd++) n_in += __builtin_popcountll(bm[wd]);
            std::vector<float> cs;
            for (int k = 0; k < n_cand; k++) {
                cs.clear();
                for (int i = 0; i < N; i++) if (flags[(size_t)k * N + i] & 1) cs.push_back(cosv[(size_t)k * N + i]);
                nGood[k] = (int32_t)cs.size();
                parallax[k] = parallax_of(cs);
            }
            chosen = model == 0 ? decide_h(nGood, parallax, n_in, pb->min_parallax, pb->min_triangulated)
                                : decide_f(nGood, parallax, n_in, pb->min_parallax, pb->min_triangulated);
        }

        // ---- outputs
        clear_outputs();
        res->model = model; res->score_h = SH; res->score_f = SF; res->best_h = best_h; res->best_f = best_f;
        if (chosen >= 0) {
            res->initialized = 1;
            std::memcpy(res->R21, R.cand[chosen].R, 36); std::memcpy(res->t21, R.cand[chosen].t, 12);
            for (int i = 0; i < N; i++) {
                const size_t o = (size_t)chosen * N + i;
                if (!(flags[o] & 1)) continue;
                std::memcpy(p3d + 3 * (size_t)m1[i], X + 3 * o, 12);          // :885
                tri[m1[i]] = (flags[o] >> 1) & 1;                           // :888
            }
        }
        if (tap) {
            G.get(tap->H21, o_h21, (size_t)iters * 36); G.get(tap->H12, o_h12, (size_t)iters * 36); G.get(tap->F21, o_f21, (size_t)iters * 36);
            G.get(tap->score_h, o_sh, (size_t)iters * 4); G.get(tap->score_f, o_sf, (size_t)iters * 4);
            G.get(tap->mask_h, o_mh, (size_t)iters * words * 8); G.get(tap->mask_f, o_mf, (size_t)iters * words * 8);
            if (tap->sets) std::memcpy(tap->sets, sets.data(), sets.size() * 4);
            tap->n_candidates = n_cand;
            for (int k = 0; k < INI_MAX_CAND; k++) {
                const bool on = k < n_cand;
                for (int e = 0; e < 9; e++) tap->cand_R[k][e] = on ? R.cand[k].R[e] : 0.0f;
                for (int e = 0; e < 3; e++) tap->cand_t[k][e] = on ? R.cand[k].t[e] : 0.0f;
                tap->cand_n_good[k] = nGood[k]; tap->cand_parallax[k] = parallax[k];
            }
            const size_t live = (size_t)n_cand * N, all = (size_t)INI_MAX_CAND * N;
            if (tap->cand_flags) { std::memcpy(tap->cand_flags, flags, live); std::memset(tap->cand_flags + live, 0, all - live); }
            if (tap->cand_cos) { std::memcpy(tap->cand_cos, cosv, live * 4); std::memset(tap->cand_cos + live, 0, (all - live) * 4); }
            if (tap->cand_p3d) { std::memcpy(tap->cand_p3d, X, live * 12); std::memset(tap->cand_p3d + 3 * live, 0, (all - live) * 12); }
        }
        return CCM_OK;
    });
}
