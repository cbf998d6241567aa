// init_kernels.hip -- the two launches of ccm_initialize (src/Initializer.cpp).
//
// k_init_hypotheses: every minimal set of FindHomography / FindFundamental (:144-167, :195-218) at once.  The 2 x mMaxIterations
// hypotheses do not depend on each other; "keep the first strictly best score" is a scan over one float per hypothesis and stays on
// the host (init_host.cpp).  A workgroup takes INI_SPB sets: waves 0-1 the homographies, waves 2-3 the fundamental matrices, one
// hypothesis per group of 16 lanes.  The null vector of the 16x9 / 8x9 float matrix A comes from a cyclic Jacobi in double on A^T A;
// its 9x9 and the 9x9 of eigenvectors (162 doubles) would spill from one lane's registers, so A, A^T A and V live in LDS and lane k of
// the group owns row k (first half of a rotation) and column k (second half), with a wave-level synchronisation between the halves.
// The matches are then staged in LDS as structure-of-arrays and the four waves take the 16 hypotheses in turn: the matrix is read
// from LDS (a broadcast), lanes stride over the matches, __ballot gives a mask word.  Each lane adds its terms in match order and a
// fixed shuffle tree adds the lanes: no atomics, the same bits on every call.
//
// k_init_check_rt: CheckRT (:794-903) of all 4 or 8 motion hypotheses of ReconstructF / ReconstructH in one launch, one thread per
// (candidate, match); the 4x4 of Triangulate fits one lane's registers.  The counts, the parallax and the decisions are the host's.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "init_types.h"
#include "init_math.h"

// LDS writes of this wave's lanes become visible to its other lanes (the hardware executes a wave's LDS instructions in order; this
// keeps the compiler from moving accesses across the point).  It is called under divergent control flow: the four groups of a wave
// skip rotations independently.  That is sound because only the 16 lanes of one group exchange data, they read the same three
// entries and so always take the same branch, and groups share no LDS.
__device__ __forceinline__ void ini_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(INI_TPB) void k_init_hypotheses(IniDev D)
{
    constexpr int G = INI_TPB / INI_GROUP;            // 16 hypotheses per workgroup
    __shared__ float sA[G][16 * 9];                   // the design matrix, row-major (rows 8..15 are zero for F)
    __shared__ double sM[G][81], sV[G][81];           // A^T A and the accumulated rotations
    __shared__ float sMat[G][18];                     // H21 | H12, or F21
    __shared__ float su1[INI_TILE], sv1[INI_TILE], su2[INI_TILE], sv2[INI_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = tid / INI_GROUP, c = tid % INI_GROUP;
    const bool isF = grp >= INI_SPB;
    const int it_raw = blockIdx.x * INI_SPB + (grp & (INI_SPB - 1));
    const bool active = it_raw < D.iters;
    const int it = active ? it_raw : D.iters - 1;     // an idle group repeats the last set and stores nothing: no divergence inside a wave

    // ---- the design matrix: lane c builds row c from the normalised points of Normalize (:767-783)
    {
        const int pt = isF ? (c & 7) : (c >> 1);
        const int idx = D.sets[8 * it + pt];
        const float* mm = D.m + 4 * (size_t)idx;
        const float u1 = (mm[0] - D.T1[2]) * D.T1[0], v1 = (mm[1] - D.T1[3]) * D.T1[1];
        const float u2 = (mm[2] - D.T2[2]) * D.T2[0], v2 = (mm[3] - D.T2[3]) * D.T2[1];
        float a[9];
        if (isF) { ini_row_f(u1, v1, u2, v2, a); if (c >= 8) { for (int k = 0; k < 9; k++) a[k] = 0.0f; } }
        else ini_row_h(c, u1, v1, u2, v2, a);
#pragma unroll
        for (int k = 0; k < 9; k++) sA[grp][9 * c + k] = a[k];
    }
    ini_wave_sync();
    double* M = sM[grp]; double* V = sV[grp];
    if (c < 9) {                                      // row c of A^T A: exact products of floats, summed in double in row order
        for (int j = 0; j < 9; j++) {
            double acc = 0.0;
            for (int r = 0; r < 16; r++) acc += (double)sA[grp][9 * r + c] * (double)sA[grp][9 * r + j];
            M[9 * c + j] = acc; V[9 * c + j] = c == j ? 1.0 : 0.0;
        }
    }
    ini_wave_sync();
    // ---- cyclic Jacobi: a' = J^T a J, V' = V J
    for (int sweep = 0; sweep < INI_SWEEPS; sweep++)
        for (int p = 0; p < 8; p++)
            for (int q = p + 1; q < 9; q++) {
                const double app = M[9 * p + p], aqq = M[9 * q + q], apq = M[9 * p + q];
                if (ini_negligible(app, aqq, apq)) continue;          // the same decision in all 16 lanes of the group
                double cs, sn;
                ini_rotation(app, aqq, apq, &cs, &sn);
                if (c < 9) ini_jacobi9_row(M, V, c, p, q, cs, sn);      // a J and V J: row c
                ini_wave_sync();
                if (c < 9) ini_jacobi9_col(M, c, p, q, cs, sn);         // J^T (a J): column c
                ini_wave_sync();
            }
    // ---- the eigenvector of the smallest eigenvalue, then :155-157 / :292-298, :208 (every lane of the group; lane 0 stores)
    {
        const int jmin = ini_jacobi9_smallest(M);
        double x[9];
#pragma unroll
        for (int k = 0; k < 9; k++) x[k] = V[9 * k + jmin];
        float A0[9], A1[9];
        if (isF) ini_finish_f(x, D.T1, D.T2, A0);
        else ini_finish_h(x, D.T1, D.T2, A0, A1);
        if (c == 0) {
#pragma unroll
            for (int k = 0; k < 9; k++) { sMat[grp][k] = A0[k]; sMat[grp][9 + k] = isF ? 0.0f : A1[k]; }
            if (active) {
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    if (isF) D.F21[9 * (size_t)it + k] = A0[k];
                    else { D.H21[9 * (size_t)it + k] = A0[k]; D.H12[9 * (size_t)it + k] = A1[k]; }
                }
            }
        }
    }

    // ---- CheckHomography / CheckFundamental of the workgroup's 16 hypotheses over all matches
    float part[G / 4];                                // this lane's share of the score of hypothesis wave + 4 k
#pragma unroll
    for (int k = 0; k < G / 4; k++) part[k] = 0.0f;
    for (int t0 = 0; t0 < D.n; t0 += INI_TILE) {
        const int nt = min(INI_TILE, D.n - t0);
        __syncthreads();                              // the last pass' readers are done (and sMat is written)
        for (int l = tid; l < nt; l += INI_TPB) {
            const float* mm = D.m + 4 * (size_t)(t0 + l);
            su1[l] = mm[0]; sv1[l] = mm[1]; su2[l] = mm[2]; sv2[l] = mm[3];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < G / 4; k++) {
            const int hh = wave + 4 * k;              // k < 2: a homography, else a fundamental matrix (the same for the whole wave)
            const int hit = blockIdx.x * INI_SPB + (hh & (INI_SPB - 1));
            if (hit >= D.iters) continue;
            const bool hF = hh >= INI_SPB;
            float A0[9], A1[9];
#pragma unroll
            for (int e = 0; e < 9; e++) { A0[e] = sMat[hh][e]; A1[e] = sMat[hh][9 + e]; }
            unsigned long long* mw = (hF ? D.mask_f : D.mask_h) + (size_t)hit * D.words + t0 / 64;
            float acc = part[k];
            for (int l0 = 0; l0 < nt; l0 += 64) {
                const int l = l0 + lane;
                bool in = false;
                if (l < nt) {
                    float s1, s2;
                    if (hF) ini_check_f(A0, su1[l], sv1[l], su2[l], sv2[l], D.inv_sigma2, &in, &s1, &s2);
                    else ini_check_h(A0, A1, su1[l], sv1[l], su2[l], sv2[l], D.inv_sigma2, &in, &s1, &s2);
                    acc += s1; acc += s2;
                }
                const unsigned long long m = __ballot(in);
                if (lane == 0) mw[l0 / 64] = m;
            }
            part[k] = acc;
        }
    }
#pragma unroll
    for (int k = 0; k < G / 4; k++) {
        const int hh = wave + 4 * k;
        const int hit = blockIdx.x * INI_SPB + (hh & (INI_SPB - 1));
        float s = part[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0 && hit < D.iters) (hh >= INI_SPB ? D.score_f : D.score_h)[hit] = s;
    }
}

__global__ __launch_bounds__(INI_RT_TPB) void k_init_check_rt(IniRtDev D)
{
    const int i = blockIdx.x * INI_RT_TPB + threadIdx.x, k = blockIdx.y;
    if (i >= D.n) return;
    const size_t o = (size_t)k * D.n + i;
    int f = 0; float X[3] = { 0.0f, 0.0f, 0.0f }, cosp = 0.0f;
    if (D.mask[i >> 6] >> (i & 63) & 1) {             // :828
        const float* mm = D.m + 4 * (size_t)i;
        const IniCand& C = D.cand[k];
        f = ini_check_rt(D.K, C.R, C.t, C.O2, C.P2, D.th2, mm[0], mm[1], mm[2], mm[3], X, &cosp);
    }
    D.flags[o] = (uint8_t)f; D.cosp[o] = cosp;
    D.X[3 * o] = X[0]; D.X[3 * o + 1] = X[1]; D.X[3 * o + 2] = X[2];
}

void init_hypotheses_launch(hipStream_t s, const IniDev& D)
{
    hipLaunchKernelGGL(k_init_hypotheses, dim3((D.iters + INI_SPB - 1) / INI_SPB), dim3(INI_TPB), 0, s, D);
}
void init_check_rt_launch(hipStream_t s, const IniRtDev& D)
{
    hipLaunchKernelGGL(k_init_check_rt, dim3((D.n + INI_RT_TPB - 1) / INI_RT_TPB, D.n_cand), dim3(INI_RT_TPB), 0, s, D);
}
