// ba_pcg.hip -- the classic preconditioned conjugate gradient iteration on the packed blocks of the reduced camera system.
//
// The reduced system is solved by block-Jacobi preconditioned conjugate gradients on the packed blocks
// (stand-in for LinearSolverEigen's sparse LDLT, solvers/linear_solver_eigen.h:106-136; converged to a
// relative residual of 1e-13 it agrees with the exact solve far below the 1e-5 pose tolerance); small
// systems and non-converging ones are scattered into a dense array and go to the dense solve (ba_dense.hip).  The preconditioner's
// two levels are built in ba_pcg_precond.hip; the pipelined form of the iteration is ba_ppcg.hip.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ba_types.h"
#include "ba_launch.h"
#include "ba_pcg.h"

// P^T r comes from the kernels that make r (k_pcg_init, k_pcg_update): a block of PCG_UPD_TPB scalars is PCG_UPD_KF consecutive
// keyframes, which touch at most PCG_RSLOTS consecutive aggregates (the first is pcg_hat(first keyframe).i0); thread (slot, d) walks
// the block's keyframes in order and leaves its partial sum in rpart[block][slot][d].  k_pcg_coarse adds the two or three blocks
// of an aggregate in block order: fixed summation order, no extra launch (a kernel of its own took 15 us per PCG iteration).
#define PCG_RSLOTS 4          // PCG_UPD_KF / (aggregate >= 16 keyframes) + 2
__device__ __forceinline__ void pcg_block_restrict(const double* rs, int nfree, int nagg, const double* __restrict__ svec, const double* __restrict__ cen,
                                                   double* __restrict__ rpart)
{
    if (!rpart) return;                                            // (uniform: no coarse level in this solve)
    // every thread (keyframe k of the block, component d) weights its residual for the keyframe's two aggregates; the thread of
    // component 3 also forms the scale products; then thread (slot, d) adds the block's keyframes in order
    __shared__ double cw[2][PCG_UPD_KF][PCG_CDOF];
    __shared__ int ci0[PCG_UPD_KF], ci1[PCG_UPD_KF];
    const int A = PCG_CL * pcg_agg_clusters(nfree);
    const int f0 = blockIdx.x * PCG_UPD_KF;
    {
        const int k = threadIdx.x / 6, d = threadIdx.x - 6 * k, f = f0 + k;
        if (f < nfree) {
            const PcgHat h = pcg_hat(f, A, nagg);
            const double r = rs[threadIdx.x];
            cw[0][k][d] = h.w0 * r; cw[1][k][d] = h.w1 * r;
            if (d == 3) {
                const double* t = svec + 3LL * f; const double* c0 = cen + 3 * h.i0; const double* c1 = cen + 3 * h.i1;
                const double* rf = rs + 6 * k + 3;
                cw[0][k][6] = h.w0 * (((t[0] - c0[0]) * rf[0] + (t[1] - c0[1]) * rf[1]) + (t[2] - c0[2]) * rf[2]);
                cw[1][k][6] = h.w1 * (((t[0] - c1[0]) * rf[0] + (t[1] - c1[1]) * rf[1]) + (t[2] - c1[2]) * rf[2]);
                ci0[k] = h.i0; ci1[k] = h.i1;
            }
        } else if (d == 3) { ci0[k] = -1; ci1[k] = -1; }
    }
    __syncthreads();
    if (threadIdx.x < PCG_RSLOTS * PCG_CDOF) {
        const int slot = threadIdx.x / PCG_CDOF, d = threadIdx.x - PCG_CDOF * slot;
        const int I = pcg_hat(f0, A, nagg).i0 + slot;
        double s = 0.0;
#pragma unroll 8
        for (int k = 0; k < PCG_UPD_KF; k++) {                       // branch-free, so that the LDS reads of several keyframes are in flight (x + 0.0 == x)
            const int j0 = ci0[k], j1 = ci1[k];
            const double a0 = cw[0][k][d], a1 = cw[1][k][d];
            s += j0 == I ? a0 : 0.0;
            s += (j1 == I && j1 != j0) ? a1 : 0.0;
        }
        rpart[((long long)blockIdx.x * PCG_RSLOTS + slot) * PCG_CDOF + d] = s;
    }
}
// yc = Ac^-1 (P^T r), one wave per row; cpart = the workgroup's share of (P^T r) . yc  (= r . (P yc), the coarse part of r.z)
__global__ __launch_bounds__(256) void k_pcg_coarse(const double* __restrict__ Aci, int nc, int ncp, const double* __restrict__ rpart, int nfree,
                                                    double* __restrict__ yc, double* __restrict__ cpart)
{
    extern __shared__ double rc[];
    __shared__ double dots[4];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, row = blockIdx.x * 4 + wv;
    // the row of the inverse is requested first: its latency passes under the copy of P^T r
    constexpr int PRE = 24;                                   // 64 * 24 = 1536 columns in registers, the rest (larger maps) afterwards
    double av[PRE];
    const double* A = Aci + (long long)min(row, nc - 1) * ncp;
#pragma unroll
    for (int q = 0; q < PRE; q++) { const int c = lane + 64 * q; av[q] = c < nc ? A[c] : 0.0; }
    {
        const int A = PCG_CL * pcg_agg_clusters(nfree), nagg = nc / PCG_CDOF;
        for (int i = threadIdx.x; i < nc; i += 256) {
            const int I = i / PCG_CDOF, d = i - PCG_CDOF * I;
            int f0, f1;
            pcg_hat_support(I, A, nfree, f0, f1);
            double sum = 0.0;
            for (int b = f0 / PCG_UPD_KF; b <= (f1 - 1) / PCG_UPD_KF; b++) {            // the blocks of k_pcg_update that hold keyframes of I
                const int slot = I - pcg_hat(b * PCG_UPD_KF, A, nagg).i0;
                if (slot >= 0 && slot < PCG_RSLOTS) sum += rpart[((long long)b * PCG_RSLOTS + slot) * PCG_CDOF + d];
            }
            rc[i] = sum;
        }
    }
    __syncthreads();
    double s = 0;
    if (row < nc) {
#pragma unroll
        for (int q = 0; q < PRE; q++) { const int c = lane + 64 * q; if (c < nc) s += av[q] * rc[c]; }
        for (int c = lane + 64 * PRE; c < nc; c += 64) s += A[c] * rc[c];
    }
    for (int st = 32; st >= 1; st >>= 1) s += __shfl_xor(s, st, 64);
    if (lane == 0) { if (row < nc) yc[row] = s; dots[wv] = row < nc ? s * rc[row] : 0.0; }
    __syncthreads();
    if (threadIdx.x == 0) cpart[blockIdx.x] = ((dots[0] + dots[1]) + dots[2]) + dots[3];
}
// yc = Ac^-1 P^T r  (P^T r as block partials in C.rc, left there by k_pcg_init / k_pcg_update), and the coarse share of r.z into C.cpart
static void pcg_launch_coarse(hipStream_t s, const PcgCoarse& C, int nfree, double* w)
{
    const int nagg = pcg_coarse_aggregates(nfree), nc = PCG_CDOF * nagg;
    (void)w;
    hipLaunchKernelGGL(k_pcg_coarse, dim3(nblk(nc, 4)), dim3(256), (size_t)nc * 8, s, C.Aci, nc, pcg_coarse_pitch(nfree), C.rc, nfree, C.yc, C.cpart);
}

// The new search direction, one thread per scalar unknown:  p = (z + P yc) + beta p,  beta = r.z (now) / r.z (previous iteration).
// Every workgroup re-reduces the partial sums of r.z (cluster part from k_pcg_init / k_pcg_update, coarse part from k_pcg_coarse) in
// the same fixed order; the previous value comes from the alternating slot sc[8 + (parity ^ 1)], and block 0 leaves the current
// one in sc[8 + parity] for k_pcg_update and the next iteration, together with the scalars the host looks at.  yc == nullptr: no
// coarse level in this solve.
__global__ __launch_bounds__(256) void k_pcg_direction(const double* __restrict__ yc, const double* __restrict__ svec, const double* __restrict__ cen,
                                                       int nfree, int nagg, double* __restrict__ w, int nblk_part, const double* __restrict__ part,
                                                       const double* __restrict__ cpart, int ncpart, double* __restrict__ sc, int parity)
{
    __shared__ double s_beta;
    if (threadIdx.x < 64) {
        double rz = 0, rr = 0;
        for (int i = threadIdx.x; i < nblk_part; i += 64) { rz += part[3 * i]; rr += part[3 * i + 1]; }
        double rzc = 0;
        for (int i = threadIdx.x; i < ncpart; i += 64) rzc += cpart[i];
        for (int st = 32; st >= 1; st >>= 1) { rz += __shfl_xor(rz, st, 64); rr += __shfl_xor(rr, st, 64); rzc += __shfl_xor(rzc, st, 64); }
        rz += rzc;
        if (threadIdx.x == 0) {
            const double rz_prev = sc[8 + (parity ^ 1)];
            s_beta = rz_prev > 0.0 ? rz / rz_prev : 0.0;
            if (blockIdx.x == 0) {                                 // scalars for k_pcg_update, the next iteration and the host
                const double pap = part[2];
                sc[8 + parity] = rz;
                sc[0] = rz; sc[2] = rr; if (pap < sc[3]) sc[3] = pap; sc[4] += 1.0;
            }
        }
    }
    __syncthreads();
    const long long n = 6LL * nfree;
    const long long o = blockIdx.x * 256LL + threadIdx.x;
    if (o >= n) return;
    double zf = w[2 * n + o];
    if (yc) {
        const int f = (int)(o / 6), d = (int)(o - 6LL * f);
        const PcgHat h = pcg_hat(f, PCG_CL * pcg_agg_clusters(nfree), nagg);
        const double* y0 = yc + PCG_CDOF * h.i0; const double* y1 = yc + PCG_CDOF * h.i1;
        double v = h.w0 * y0[d] + h.w1 * y1[d];
        if (d >= 3) {
            const double t = svec[3LL * f + (d - 3)];
            v += h.w0 * ((t - cen[3 * h.i0 + (d - 3)]) * y0[6]) + h.w1 * ((t - cen[3 * h.i1 + (d - 3)]) * y1[6]);
        }
        zf += v;
    }
    w[3 * n + o] = zf + s_beta * w[3 * n + o];
}
// p = (z + P yc) + beta p and the scalars of the iteration; parity = the r.z slot this call writes
static void pcg_launch_direction(hipStream_t s, const PcgCoarse& C, int nfree, double* w, double* part, double* sc, int parity)
{
    const long long n = 6LL * nfree;
    hipLaunchKernelGGL(k_pcg_direction, dim3(nblk(n, 256)), dim3(256), 0, s, C.Aci ? C.yc : nullptr, C.svec, C.cen, nfree, C.Aci ? pcg_coarse_aggregates(nfree) : 0, w,
                       nblk(n, PCG_UPD_TPB), part, C.cpart, C.Aci ? pcg_coarse_parts(nfree) : 0, sc, parity);
}

// state vector layout in `w`: x | r | z (cluster level only) | p | Ap  (each n doubles); scalars in sc[]:
//   sc[0] rz, sc[1] |b|^2, sc[2] |r|^2, sc[3] min p.Ap seen, sc[4] iterations
static_assert(PCG_UPD_TPB % PCG_CN == 0, "a block must hold whole clusters");
__global__ __launch_bounds__(PCG_UPD_TPB) void k_pcg_init(const double* __restrict__ b, const double* __restrict__ Minv, int nfree,
                                                          double* __restrict__ w, double* __restrict__ part, int nagg, const double* __restrict__ svec,
                                                          const double* __restrict__ cen, double* __restrict__ rpart)
{
    __shared__ double rs[PCG_UPD_TPB];
    __shared__ double red[2][3];
    const long long n = 6LL * nfree;
    const long long o = (long long)blockIdx.x * PCG_UPD_TPB + threadIdx.x;
    const double ri = o < n ? b[o] : 0.0;
    rs[threadIdx.x] = ri;
    __syncthreads();
    pcg_block_restrict(rs, nfree, nagg, svec, cen, rpart);
    double rz = 0, bb = 0;
    if (o < n) {
        const int cl = (int)(o / PCG_CN), li = (int)(o - (long long)cl * PCG_CN), base = (threadIdx.x / PCG_CN) * PCG_CN;
        const double* M = Minv + (long long)cl * PCG_CN * PCG_CN + li;
        double z = 0;
#pragma unroll 8
        for (int k = 0; k < PCG_CN; k++) z += M[k * PCG_CN] * rs[base + k];       // symmetric: column li read with unit stride across lanes
        w[o] = 0.0; w[n + o] = ri; w[2 * n + o] = z; w[3 * n + o] = 0.0;                         // p = z + beta * 0 in the first direction
        rz = ri * z; bb = ri * ri;
    }
    for (int s = 32; s >= 1; s >>= 1) { rz += __shfl_xor(rz, s, 64); bb += __shfl_xor(bb, s, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = rz; red[1][threadIdx.x >> 6] = bb; }
    __syncthreads();
    if (threadIdx.x == 0) {                   // same layout as k_pcg_update: r.z, |r|^2, p.Ap
        part[3 * blockIdx.x] = (red[0][0] + red[0][1]) + red[0][2];
        part[3 * blockIdx.x + 1] = (red[1][0] + red[1][1]) + red[1][2];
        part[3 * blockIdx.x + 2] = 1e300;
    }
}
__global__ __launch_bounds__(64) void k_pcg_init_fin(const double* __restrict__ part, int nblk, const double* __restrict__ cpart, int ncpart,
                                                     double* __restrict__ sc)
{
    if (threadIdx.x != 0) return;
    double rz = 0, bb = 0, rzc = 0;
    for (int i = 0; i < nblk; i++) { rz += part[3 * i]; bb += part[3 * i + 1]; }
    for (int i = 0; i < ncpart; i++) rzc += cpart[i];
    rz += rzc;
    sc[0] = rz; sc[1] = bb; sc[2] = bb; sc[3] = 1e300; sc[4] = -1.0; sc[8] = rz; sc[9] = rz;      // (the direction call of the start-up adds 1)
}
// rpart of k_pcg_init / k_pcg_update: PCG_RSLOTS x PCG_CDOF partials per block of PCG_UPD_TPB scalars (two blocks of slack)
size_t pcg_coarse_rpart_doubles(int nfree) { return ((size_t)(6LL * nfree) / PCG_UPD_TPB + 2) * PCG_RSLOTS * PCG_CDOF; }
// part: three partial sums per keyframe and per block of PCG_UPD_TPB scalars (four blocks of slack)
size_t pcg_part_doubles(int nfree) { return ((size_t)nfree + (size_t)(6LL * nfree) / PCG_UPD_TPB + 4) * 3; }
void pcg_launch_init(hipStream_t s, const double* b, const double* Minv, int nfree, double* w, double* part, double* sc, const PcgCoarse& C)
{
    const int nb = nblk(6LL * nfree, PCG_UPD_TPB);
    hipLaunchKernelGGL(k_pcg_init, dim3(nb), dim3(PCG_UPD_TPB), 0, s, b, Minv, nfree, w, part, C.Aci ? pcg_coarse_aggregates(nfree) : 0, C.svec, C.cen,
                       C.Aci ? C.rc : nullptr);
    if (C.Aci) pcg_launch_coarse(s, C, nfree, w);
    hipLaunchKernelGGL(k_pcg_init_fin, dim3(1), dim3(64), 0, s, part, nb, C.cpart, C.Aci ? pcg_coarse_parts(nfree) : 0, sc);
    pcg_launch_direction(s, C, nfree, w, part, sc, 1);          // "iteration -1": beta = r.z / r.z with p = 0, i.e. p = z + P yc
}

// Ap = A p, one workgroup per block row (p comes from k_pcg_direction).
// Thread = (entry slot 0..41, row component 0..5); the 42 slot sums of a component are added in slot order by one lane.
__global__ __launch_bounds__(256) void k_pcg_spmv(const double* __restrict__ Hb, const int* __restrict__ row_ptr, const unsigned* __restrict__ ent_key,
                                                  const unsigned* __restrict__ ent_val, int nfree, double* __restrict__ w, double* __restrict__ pap_part)
{
    __shared__ double red[42][6];
    // Workgroups are dealt round-robin to the 8 XCDs, so b and b + 8 share an L2.  Giving each XCD a contiguous range of
    // block rows means that block (i, j) of the band, needed by row i and (transposed) by row j a few rows later, is
    // fetched from the fabric once and found in that XCD's L2 the second time.
    const int rows_per_xcd = (nfree + PCG_XCDS - 1) / PCG_XCDS;
    const int row = ((int)blockIdx.x % PCG_XCDS) * rows_per_xcd + (int)blockIdx.x / PCG_XCDS;
    if (row >= nfree) return;
    const long long n = 6LL * nfree;
    const double* p = w + 3 * n;
    const int slot = threadIdx.x / 6, r = threadIdx.x - 6 * slot;
    if (slot < 42) {
        double acc = 0;
        const int k_end = row_ptr[2 * row + 1];
        // four entries per step: all index loads are issued first, then all block / vector loads, so a row of
        // up to 168 blocks costs two dependent memory round trips instead of eight
        for (int k0 = row_ptr[2 * row] + slot; k0 < k_end; k0 += 4 * 42) {
            unsigned v[4]; int col[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int k = k0 + 42 * q;
                v[q] = 0xFFFFFFFFu; col[q] = 0;
                if (k < k_end) { v[q] = ent_val[k]; col[q] = (int)(ent_key[k] - (unsigned)row * (unsigned)nfree); }
            }
            double bv[4][6], xv[4][6];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (v[q] == 0xFFFFFFFFu) {
#pragma unroll
                    for (int c = 0; c < 6; c++) { bv[q][c] = 0; xv[q][c] = 0; }
                    continue;
                }
                const double* B = Hb + 36 * (long long)(v[q] & 0x7FFFFFFFu);
                const double* pc = p + 6 * (long long)col[q];
                const bool tr = (v[q] & 0x80000000u) != 0u;
#pragma unroll
                for (int c = 0; c < 6; c++) { bv[q][c] = tr ? B[c * 6 + r] : B[r * 6 + c]; xv[q][c] = pc[c]; }
            }
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int c = 0; c < 6; c++) acc += bv[q][c] * xv[q][c];
        }
        red[slot][r] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        double tot = 0, pap = 0;
        if (threadIdx.x < 6) {
            for (int s2 = 0; s2 < 42; s2++) tot += red[s2][threadIdx.x];
            const long long o = 6LL * row + threadIdx.x;
            w[4 * n + o] = tot;
            pap = tot * p[o];
        }
        for (int st = 4; st >= 1; st >>= 1) pap += __shfl_xor(pap, st, 64);     // lanes 0..7 (6,7 hold 0)
        if (threadIdx.x == 0) pap_part[row] = pap;
    }
}

// x += alpha p; r -= alpha Ap; z = Minv r (cluster mat-vec); partial r.z and r.r.  One thread per scalar unknown, a
// block holds 4 whole clusters whose new residuals are shared through LDS.  Every block re-reduces p.Ap itself.
__global__ __launch_bounds__(PCG_UPD_TPB) void k_pcg_update(const double* __restrict__ Minv, int nfree, double* __restrict__ w,
                                                            const double* __restrict__ pap_part, const double* __restrict__ sc, double* __restrict__ part,
                                                            int parity, int nagg, const double* __restrict__ svec, const double* __restrict__ cen,
                                                            double* __restrict__ rpart)
{
    __shared__ double red[4];
    __shared__ double red2[2][3];
    __shared__ double rs[PCG_UPD_TPB];
    const long long n = 6LL * nfree;
    const long long o = (long long)blockIdx.x * PCG_UPD_TPB + threadIdx.x;
    // everything this thread needs is requested before the reduction, so that all global loads overlap
    double r_old = 0, ap = 0, x_old = 0, p_old = 0;
    double mv[PCG_CN];                                              // this unknown's column of its cluster inverse: 48 loads that wait for nothing
    if (o < n) {
        r_old = w[n + o]; ap = w[4 * n + o]; x_old = w[o]; p_old = w[3 * n + o];   // this iteration's direction
        const int cl = (int)(o / PCG_CN), li = (int)(o - (long long)cl * PCG_CN);
        const double* M = Minv + (long long)cl * PCG_CN * PCG_CN + li;
#pragma unroll
        for (int k = 0; k < PCG_CN; k++) mv[k] = M[k * PCG_CN];    // symmetric: column li read with unit stride across lanes
    }
    const double rz_old = sc[8 + (parity ^ 1)];                     // this iteration's r.z, left there by k_pcg_direction
    double s = 0;
#pragma unroll 4
    for (int k = threadIdx.x; k < nfree; k += PCG_UPD_TPB) s += pap_part[k];
    for (int st = 32; st >= 1; st >>= 1) s += __shfl_xor(s, st, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const double pap = (red[0] + red[1]) + red[2];
    const double alpha = pap > 0.0 ? rz_old / pap : 0.0;
    const double ri = r_old - alpha * ap;
    rs[threadIdx.x] = ri;
    __syncthreads();
    pcg_block_restrict(rs, nfree, nagg, svec, cen, rpart);
    double rz = 0, rr = 0;
    if (o < n) {
        const int base = (threadIdx.x / PCG_CN) * PCG_CN;
        double z = 0;
#pragma unroll
        for (int k = 0; k < PCG_CN; k++) z += mv[k] * rs[base + k];
        w[o] = x_old + alpha * p_old; w[n + o] = ri; w[2 * n + o] = z;
        rz = ri * z; rr = ri * ri;
    }
    for (int st = 32; st >= 1; st >>= 1) { rz += __shfl_xor(rz, st, 64); rr += __shfl_xor(rr, st, 64); }
    if ((threadIdx.x & 63) == 0) { red2[0][threadIdx.x >> 6] = rz; red2[1][threadIdx.x >> 6] = rr; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x] = (red2[0][0] + red2[0][1]) + red2[0][2];
        part[3 * blockIdx.x + 1] = (red2[1][0] + red2[1][1]) + red2[1][2];
        part[3 * blockIdx.x + 2] = pap;
    }
}
// one PCG iteration = mat-vec, the vector updates with the cluster level, the coarse level, the next direction
void pcg_launch_iter(hipStream_t s, const double* Hb, const int* row_ptr, const unsigned* ekey, const unsigned* eval, const double* Minv,
                     int nfree, double* w, double* pap_part, double* part, double* sc, int parity, const PcgCoarse& C)
{
    const int nb = nblk(6LL * nfree, PCG_UPD_TPB);
    hipLaunchKernelGGL(k_pcg_spmv, dim3(PCG_XCDS * nblk(nfree, PCG_XCDS)), dim3(256), 0, s, Hb, row_ptr, ekey, eval, nfree, w, pap_part);
    hipLaunchKernelGGL(k_pcg_update, dim3(nb), dim3(PCG_UPD_TPB), 0, s, Minv, nfree, w, pap_part, sc, part, parity, C.Aci ? pcg_coarse_aggregates(nfree) : 0,
                       C.svec, C.cen, C.Aci ? C.rc : nullptr);
    if (C.Aci) pcg_launch_coarse(s, C, nfree, w);
    pcg_launch_direction(s, C, nfree, w, part, sc, parity);
}

__global__ __launch_bounds__(64) void k_pcg_scalars(int nblk, const double* __restrict__ part, const double* __restrict__ cpart, int ncpart,
                                                    double* __restrict__ sc)
{
    // the same sums in the same order as a workgroup of k_pcg_spmv forms them (one thread walking the ~300 partials took 20 us)
    double rz = 0, rr = 0, rzc = 0;
    for (int i = threadIdx.x; i < nblk; i += 64) { rz += part[3 * i]; rr += part[3 * i + 1]; }
    for (int i = threadIdx.x; i < ncpart; i += 64) rzc += cpart[i];
    for (int st = 32; st >= 1; st >>= 1) { rz += __shfl_xor(rz, st, 64); rr += __shfl_xor(rr, st, 64); rzc += __shfl_xor(rzc, st, 64); }
    if (threadIdx.x != 0) return;
    rz += rzc;
    const double pap = part[2];
    sc[0] = rz; sc[2] = rr; if (pap < sc[3]) sc[3] = pap; sc[4] += 1.0;
}
// publish the scalars of the last iteration (before the host reads them)
void pcg_launch_publish(hipStream_t s, int nfree, double* part, double* sc, const PcgCoarse& C)
{
    hipLaunchKernelGGL(k_pcg_scalars, dim3(1), dim3(64), 0, s, nblk(6LL * nfree, PCG_UPD_TPB), part, C.cpart, C.Aci ? pcg_coarse_parts(nfree) : 0, sc);
}
