// pnp_kernels.hip -- the two launches of the batched PnPsolver (src/PnPSolver.cpp).
//
// k_pnp_hypotheses: every minimal-set hypothesis of every solver of a batch (:176-198 per hypothesis: the sampled correspondences,
// EPnP compute_pose :468-516, CheckInliers :299-330).  A workgroup takes up to PNP_HPB hypotheses of one solver.  compute_pose is one
// long dependent chain in double, so it runs one hypothesis per LANE of wave 0.  The 12x12 matrix M^T M and its eigenvector matrix
// (288 doubles per hypothesis) do not fit in registers next to the rest of the chain, and the Jacobi iteration indexes them by (p, q):
// they live in LDS as [element][lane] -- consecutive lanes on consecutive doubles, so every access of the wave is conflict-free and
// dynamically indexed without scratch -- at the price of 16 instead of 64 hypotheses per workgroup.  A batch of 8 x 305 hypotheses is
// 153 workgroups, fewer than the device has CUs, so the narrower workgroup costs no second round.  Then the four waves sweep the
// solver's correspondences, staged in LDS tiles, against each hypothesis: __ballot gives a mask word and __popcll its share of the
// count.
//
// k_pnp_refine: every Refine() (:251-296) that a calling pattern can reach, one wave per (solver, record hypothesis).  The sums over
// the inlier set are taken lane-strided and reduced by a butterfly of shuffles: a fixed order, the same total in every lane, no
// atomics.  The 3x3 algebra runs redundantly in every lane (same inputs, same result, no hand-off); the 12x12 eigenproblem and the
// betas run in lane 0 on LDS.  CheckInliers then runs over all N correspondences.
//
// k_pnp_gather, in front of the two for ccm_pnp_solver_create_frames: the correspondence arrays from a frame handle and the map-point
// table (at the end of this file).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/ccm_hot.h"
#include "pnp_types.h"
#include "pnp_math.h"

// the minimal set of one hypothesis: indices in LDS ([i][lane]), the correspondences themselves from global memory
struct PnpViewSample {
    const float* P3D; const float* P2D; const int* idx; int stride;
    __device__ void get(int i, double pw[3], double uv[2]) const
    {
        const int g = idx[i * stride];
        pw[0] = P3D[3 * g]; pw[1] = P3D[3 * g + 1]; pw[2] = P3D[3 * g + 2];
        uv[0] = P2D[2 * g]; uv[1] = P2D[2 * g + 1];
    }
};

__global__ __launch_bounds__(PNP_TPB) void k_pnp_hypotheses(PnpDev D)
{
    __shared__ double sA[144 * PNP_HPB], sV[144 * PNP_HPB], sRt[12][PNP_HPB];
    __shared__ float sX[3][PNP_TILE], sU[2][PNP_TILE], sM[PNP_TILE];
    __shared__ int sidx[PNP_MAXSET][PNP_HPB], scnt[PNP_HPB];
    const PnpBlock b = D.blocks[blockIdx.x];
    const PnpSolver sv = D.solvers[b.solver];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* P3D = D.P3D + 3 * (size_t)sv.first; const float* P2D = D.P2D + 2 * (size_t)sv.first;
    const double K[4] = { sv.K[0], sv.K[1], sv.K[2], sv.K[3] };

    if (tid < b.n) {                                  // wave 0: the closed form, one hypothesis per lane
        const size_t h = (size_t)sv.hyp_first + b.hyp0 + tid;
        for (int i = 0; i < sv.min_set; i++) sidx[i][tid] = D.sample[PNP_MAXSET * h + i];      // in [0, n): checked by the host
        const PnpViewSample P{ P3D, P2D, &sidx[0][tid], PNP_HPB };
        PnpMatStrided A{ sA + tid, PNP_HPB }, V{ sV + tid, PNP_HPB };
        double Rt[12];
        pnp_compute_pose(P, sv.min_set, K, A, V, Rt, D.detail ? D.detail + PNP_DETAIL * h : nullptr);
#pragma unroll
        for (int k = 0; k < 12; k++) { sRt[k][tid] = Rt[k]; D.Rt[12 * h + k] = Rt[k]; }
        scnt[tid] = 0;
    }

    for (int t0 = 0; t0 < sv.n; t0 += PNP_TILE) {
        const int nt = min(PNP_TILE, sv.n - t0);
        __syncthreads();                              // the last pass' readers are done (and sRt / scnt are written)
        for (int l = tid; l < nt; l += PNP_TPB) {
            const int g = t0 + l;
            sX[0][l] = P3D[3 * g]; sX[1][l] = P3D[3 * g + 1]; sX[2][l] = P3D[3 * g + 2];
            sU[0][l] = P2D[2 * g]; sU[1][l] = P2D[2 * g + 1];
            sM[l] = D.max_err[sv.first + g];
        }
        __syncthreads();
        for (int hh = wave; hh < b.n; hh += PNP_TPB / 64) {
            double Rt[12];
#pragma unroll
            for (int k = 0; k < 12; k++) Rt[k] = sRt[k][hh];
            unsigned long long* mw = D.mask + sv.mask_first + ((size_t)b.hyp0 + hh) * sv.words + t0 / 64;
            int cnt = 0;
            for (int l0 = 0; l0 < nt; l0 += 64) {
                const int l = l0 + lane;
                const bool in = l < nt && pnp_inlier(Rt, K, sX[0][l], sX[1][l], sX[2][l], sU[0][l], sU[1][l], sM[l]);
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

// the same total in every lane: x_l + x_(l ^ off) is commutative, so both partners of every step hold the same bits
__device__ inline double pnp_wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

__global__ __launch_bounds__(PNP_RTPB) void k_pnp_refine(PnpRefineDev D)
{
    __shared__ double sA[144], sV[144], sBasis[4][12], sBetas[3][4];
    const PnpRecord rec = D.records[blockIdx.x];
    const PnpSolver sv = D.solvers[rec.solver];
    const int lane = threadIdx.x;
    const float* P3D = D.P3D + 3 * (size_t)sv.first; const float* P2D = D.P2D + 2 * (size_t)sv.first;
    const unsigned long long* m = D.hyp_mask + sv.mask_first + (size_t)rec.hyp * sv.words;      // mvbBestInliers
    const double K[4] = { sv.K[0], sv.K[1], sv.K[2], sv.K[3] };

    int n = 0, first = -1;                            // vIndices.size() and vIndices[0] (:256-262)
    for (int w = 0; w < sv.words; w++) {
        const unsigned long long mw = m[w];
        if (first < 0 && mw) first = 64 * w + __ffsll((long long)mw) - 1;
        n += __popcll(mw);
    }
    if (first < 0) first = 0;                         // an empty set is never a record; keep every index in range anyway
    double pw[3], uv[2], a[4];
#define PNP_LOAD(i) { pw[0] = P3D[3 * (i)]; pw[1] = P3D[3 * (i) + 1]; pw[2] = P3D[3 * (i) + 2]; uv[0] = P2D[2 * (i)]; uv[1] = P2D[2 * (i) + 1]; }
#define PNP_FOR_INLIERS for (int w = 0; w < sv.words; w++) if (m[w] >> lane & 1)

    double c0[3] = { 0, 0, 0 }, cov[6] = { 0, 0, 0, 0, 0, 0 };
    PNP_FOR_INLIERS { PNP_LOAD(64 * w + lane) c0[0] += pw[0]; c0[1] += pw[1]; c0[2] += pw[2]; }
#pragma unroll
    for (int k = 0; k < 3; k++) c0[k] = pnp_wave_sum(c0[k]) / n;
    PNP_FOR_INLIERS {
        PNP_LOAD(64 * w + lane)
        const double d0 = pw[0] - c0[0], d1 = pw[1] - c0[1], d2 = pw[2] - c0[2];
        cov[0] += d0 * d0; cov[1] += d0 * d1; cov[2] += d0 * d2; cov[3] += d1 * d1; cov[4] += d1 * d2; cov[5] += d2 * d2;
    }
#pragma unroll
    for (int k = 0; k < 6; k++) cov[k] = pnp_wave_sum(cov[k]);
    double cws[4][3], ci[3][3];
    pnp_control_points(n, c0, cov, cws, ci);

    {
        double acc[78];
#pragma unroll
        for (int k = 0; k < 78; k++) acc[k] = 0.0;
        PNP_FOR_INLIERS {
            double m1[12], m2[12];
            PNP_LOAD(64 * w + lane)
            pnp_alphas(ci, c0, pw, a);
            pnp_rows_M(a, uv, K, m1, m2);
            int e = 0;
#pragma unroll
            for (int r = 0; r < 12; r++)
#pragma unroll
                for (int c = r; c < 12; c++) acc[e++] += m1[r] * m1[c] + m2[r] * m2[c];
        }
        int e = 0;
#pragma unroll
        for (int r = 0; r < 12; r++)
#pragma unroll
            for (int c = r; c < 12; c++) {
                const double s = pnp_wave_sum(acc[e++]);
                if (lane == 0) { sA[12 * r + c] = s; sA[12 * c + r] = s; }
            }
    }
    if (lane == 0) {
        PnpMatStrided A{ sA, 1 }, V{ sV, 1 };
        pnp_jacobi12(A, V);
        pnp_basis(A, V, sBasis);
        pnp_all_betas(sBasis, cws, sBetas);
    }
    __syncthreads();
    double basis[4][12];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int k = 0; k < 12; k++) basis[r][k] = sBasis[r][k];

    double Rt[12], err[3] = { 0, 0, 0 };
    int which = 0;
    for (int cand = 0; cand < 3; cand++) {
        double betas[4], ccs[4][3], pc[3], pc0[3] = { 0, 0, 0 }, abt[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, Rc[12];
#pragma unroll
        for (int k = 0; k < 4; k++) betas[k] = sBetas[cand][k];
        pnp_ccs(betas, basis, ccs);
        PNP_LOAD(first) pnp_alphas(ci, c0, pw, a); pnp_pc(a, ccs, pc);
        pnp_sign(pc[2], ccs);
        PNP_FOR_INLIERS {
            PNP_LOAD(64 * w + lane) pnp_alphas(ci, c0, pw, a); pnp_pc(a, ccs, pc);
            pc0[0] += pc[0]; pc0[1] += pc[1]; pc0[2] += pc[2];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) pc0[k] = pnp_wave_sum(pc0[k]) / n;
        PNP_FOR_INLIERS {
            PNP_LOAD(64 * w + lane) pnp_alphas(ci, c0, pw, a); pnp_pc(a, ccs, pc);
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int k = 0; k < 3; k++) abt[3 * j + k] += (pc[j] - pc0[j]) * (pw[k] - c0[k]);
        }
#pragma unroll
        for (int k = 0; k < 9; k++) abt[k] = pnp_wave_sum(abt[k]);
        pnp_R_t(abt, pc0, c0, Rc);
        double sum2 = 0.0;
        PNP_FOR_INLIERS { PNP_LOAD(64 * w + lane) sum2 += pnp_reproj(Rc, K, pw, uv); }
        err[cand] = pnp_wave_sum(sum2) / n;
        // the choice of N (:509-511), taken as the candidates arrive
        const bool better = cand == 0 || err[cand] < err[which];
        if (better) {
            which = cand;
#pragma unroll
            for (int k = 0; k < 12; k++) Rt[k] = Rc[k];
        }
    }
#undef PNP_FOR_INLIERS
#undef PNP_LOAD

    unsigned long long* mw = D.mask + rec.mask_first;
    int cnt = 0;
    for (int l0 = 0; l0 < sv.n; l0 += 64) {
        const int l = l0 + lane;
        const bool in = l < sv.n && pnp_inlier(Rt, K, P3D[3 * l], P3D[3 * l + 1], P3D[3 * l + 2], P2D[2 * l], P2D[2 * l + 1], D.max_err[sv.first + l]);
        const unsigned long long bits = __ballot(in);
        if (lane == 0) mw[l0 / 64] = bits;
        cnt += __popcll(bits);
    }
    if (lane == 0) {
        D.count[rec.row] = cnt;
#pragma unroll
        for (int k = 0; k < 12; k++) D.Rt[12 * (size_t)rec.row + k] = Rt[k];
        if (D.detail) {
            double* d = D.detail + PNP_DETAIL * (size_t)rec.row;
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int k = 0; k < 3; k++) d[3 * j + k] = cws[j][k];
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int k = 0; k < 12; k++) d[12 + 12 * r + k] = basis[r][k];
#pragma unroll
            for (int k = 0; k < 4; k++) d[60 + k] = sBetas[which][k];
            d[64] = err[0]; d[65] = err[1]; d[66] = err[2]; d[67] = (double)(which + 1);
        }
    }
}

// The constructor's loop (:69-91) for correspondences named by (feature of a frame handle, slot of a map-point table), one thread
// each: P2D = the feature's undistorted keypoint, P3D = the slot's position, max_err = mvLevelSigma2[octave] * th2, the float product
// ccm_pnp_solver_create forms on the host (:146).  Every index is checked before it is used as an address; a feature outside the
// frame, a slot outside the table or not LIVE, or an octave outside [0, n_levels) raises status[0] (every thread that finds one stores
// the same 1) and leaves zeros, which the launch queued behind can read safely; the host then reports CCM_E_ARG.
__global__ __launch_bounds__(PNP_GTPB) void k_pnp_gather(PnpGather G)
{
    const int e = blockIdx.x * PNP_GTPB + threadIdx.x;
    if (e >= G.n) return;
    const int f = G.feature[e], s = G.slot[e];
    float u = 0.0f, v = 0.0f, X = 0.0f, Y = 0.0f, Z = 0.0f, me = 0.0f;
    bool ok = f >= 0 && f < G.n_cur && s >= 0 && s < G.capacity;
    if (ok) ok = (G.flags[s] & CCM_MP_LIVE) != 0;
    int o = 0;
    if (ok) { o = G.oct[f]; ok = o >= 0 && o < G.n_levels; }
    if (ok) {
        u = G.kx[f]; v = G.ky[f];
        X = G.pos[3 * (size_t)s]; Y = G.pos[3 * (size_t)s + 1]; Z = G.pos[3 * (size_t)s + 2];
        me = G.sigma2[o] * G.th2;
    } else G.status[0] = 1;
    G.P2D[2 * (size_t)e] = u; G.P2D[2 * (size_t)e + 1] = v;
    G.P3D[3 * (size_t)e] = X; G.P3D[3 * (size_t)e + 1] = Y; G.P3D[3 * (size_t)e + 2] = Z;
    G.max_err[e] = me;
}

void pnp_gather_launch(hipStream_t s, const PnpGather& G)
{
    if (G.n > 0) hipLaunchKernelGGL(k_pnp_gather, dim3((G.n + PNP_GTPB - 1) / PNP_GTPB), dim3(PNP_GTPB), 0, s, G);
}
void pnp_hypotheses_launch(hipStream_t s, const PnpDev& D, int n_blocks)
{
    hipLaunchKernelGGL(k_pnp_hypotheses, dim3(n_blocks), dim3(PNP_TPB), 0, s, D);
}
void pnp_refine_launch(hipStream_t s, const PnpRefineDev& D, int n_records)
{
    hipLaunchKernelGGL(k_pnp_refine, dim3(n_records), dim3(PNP_RTPB), 0, s, D);
}
