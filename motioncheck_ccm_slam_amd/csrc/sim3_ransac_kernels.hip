// sim3_ransac_kernels.hip -- every hypothesis of every Sim3Solver of a batch in ONE launch (src/Sim3Solver.cpp:146-165 per hypothesis:
// three sampled correspondences, ComputeSim3 :210-321, CheckInliers :324-348).  The hypotheses do not depend on each other; the
// ordered part of Sim3Solver::iterate (running best, first return) is a scan over one count per hypothesis and stays on the host
// (sim3_ransac_host.cpp).
//
// A workgroup takes up to S3R_HPB hypotheses of one solver.  The closed form is ~60 Jacobi rotations in double per hypothesis, a
// long dependent chain: it runs one hypothesis per LANE of wave 0 (64 at the latency of one), not once per wave.  The solver's
// correspondences are staged in LDS as structure-of-arrays (X1, X2, their own projections p1, p2 and the two bounds: 12 floats
// each), then the four waves take the hypotheses in turn: the transform is read from LDS (same address in every lane: a broadcast),
// lanes stride over the correspondences, __ballot gives a mask word and __popcll its share of the count.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sim3_ransac_types.h"
#include "sim3_ransac_math.h"

__global__ __launch_bounds__(S3R_TPB) void k_sim3_ransac(S3rDev D)
{
    __shared__ float sx1[3][S3R_TILE], sx2[3][S3R_TILE], sp1[2][S3R_TILE], sp2[2][S3R_TILE], sm1[S3R_TILE], sm2[S3R_TILE];
    __shared__ float sT[24][S3R_HPB];                 // [component][hypothesis]: T12 rows (12), T21 rows (12)
    __shared__ int scnt[S3R_HPB];
    const S3rBlock b = D.blocks[blockIdx.x];
    const S3rSolver sv = D.solvers[b.solver];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* X1 = D.X1 + 3 * (size_t)sv.first; const float* X2 = D.X2 + 3 * (size_t)sv.first;

    if (tid < b.n) {                                  // wave 0: sampling and closed form, one hypothesis per lane
        const size_t h = (size_t)sv.hyp_first + b.hyp0 + tid;
        const int r[3] = { D.draws[3 * h], D.draws[3 * h + 1], D.draws[3 * h + 2] };      // ranges checked by the host
        int idx[3];
        s3r_sample(sv.n, r, idx);
        float P1[3][3], P2[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int d = 0; d < 3; d++) { P1[i][d] = X1[3 * idx[i] + d]; P2[i][d] = X2[3 * idx[i] + d]; }
        float rts[13]; S3rXf xf;
        s3r_horn(P1, P2, sv.fix_scale != 0, rts, &xf);
#pragma unroll
        for (int k = 0; k < 12; k++) { sT[k][tid] = xf.T12[k]; sT[12 + k][tid] = xf.T21[k]; }
#pragma unroll
        for (int k = 0; k < 13; k++) D.rts[13 * h + k] = rts[k];
#pragma unroll
        for (int i = 0; i < 3; i++) D.sample[3 * h + i] = idx[i];
        scnt[tid] = 0;
    }

    for (int t0 = 0; t0 < sv.n; t0 += S3R_TILE) {
        const int nt = min(S3R_TILE, sv.n - t0);
        __syncthreads();                              // the last pass' readers are done (and sT / scnt are written)
        for (int l = tid; l < nt; l += S3R_TPB) {
            const int g = t0 + l;
            const float a0 = X1[3 * g], a1 = X1[3 * g + 1], a2 = X1[3 * g + 2];
            const float b0 = X2[3 * g], b1 = X2[3 * g + 1], b2 = X2[3 * g + 2];
            sx1[0][l] = a0; sx1[1][l] = a1; sx1[2][l] = a2; sx2[0][l] = b0; sx2[1][l] = b1; sx2[2][l] = b2;
            float u, v;
            s3r_project(nullptr, sv.K1, a0, a1, a2, &u, &v); sp1[0][l] = u; sp1[1][l] = v;      // mvP1im1 (:88)
            s3r_project(nullptr, sv.K2, b0, b1, b2, &u, &v); sp2[0][l] = u; sp2[1][l] = v;      // mvP2im2 (:89)
            sm1[l] = D.max_err1[sv.first + g]; sm2[l] = D.max_err2[sv.first + g];
        }
        __syncthreads();
        for (int hh = wave; hh < b.n; hh += S3R_TPB / 64) {
            float T12[12], T21[12];
#pragma unroll
            for (int k = 0; k < 12; k++) { T12[k] = sT[k][hh]; T21[k] = sT[12 + k][hh]; }
            unsigned long long* mw = D.mask + sv.mask_first + ((size_t)b.hyp0 + hh) * sv.words + t0 / 64;
            int cnt = 0;
            for (int l0 = 0; l0 < nt; l0 += 64) {
                const int l = l0 + lane;
                bool in = false;
                if (l < nt) {
                    float u, v;
                    s3r_project(T12, sv.K1, sx2[0][l], sx2[1][l], sx2[2][l], &u, &v);           // vP2im1 (:327)
                    const float d1x = sp1[0][l] - u, d1y = sp1[1][l] - v;
                    s3r_project(T21, sv.K2, sx1[0][l], sx1[1][l], sx1[2][l], &u, &v);           // vP1im2 (:328)
                    const float d2x = u - sp2[0][l], d2y = v - sp2[1][l];
                    const float e1 = d1x * d1x + d1y * d1y, e2 = d2x * d2x + d2y * d2y;
                    in = e1 < sm1[l] && e2 < sm2[l];                                            // :340; NaN compares false
                }
                const unsigned long long m = __ballot(in);
                if (lane == 0) mw[l0 / 64] = m;
                cnt += __popcll(m);
            }
            if (lane == 0) scnt[hh] += cnt;           // hypothesis hh always belongs to this wave
        }
    }
    __syncthreads();
    if (tid < b.n) D.count[(size_t)sv.hyp_first + b.hyp0 + tid] = scnt[tid];
}

void sim3_ransac_launch(hipStream_t s, const S3rDev& D, int n_blocks)
{
    hipLaunchKernelGGL(k_sim3_ransac, dim3(n_blocks), dim3(S3R_TPB), 0, s, D);
}
