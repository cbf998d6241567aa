// ba_schur.hip -- one LM trial's Schur complement: the block-sparse reduced camera system.
//
// What BlockSolver<6,3>::solve does per landmark (cslam/thirdparty/g2o/g2o/core/block_solver.hpp:381-432),
//     Hschur(i,j) -= Hpl(i,l) Dinv(l) Hpl(j,l)^T   for every pair i <= j of poses observing landmark l,
// is reorganised for the GPU as a GATHER: all (landmark, pose-pair) contributions are enumerated once per
// problem, sorted by their target 6x6 block (rocPRIM radix sort, stable: ba_structure.hip), and each block is then summed by
// one wave in that fixed order -- no atomics, bitwise reproducible, and the reduced system stays
// block-sparse (the covisibility pattern, ~130 blocks per keyframe row at BASELINE config 5 instead of 2000).
// The block pattern is the union over all ranks (byte map all-reduced with MAX), so every rank packs its
// partial blocks identically and one RCCL all-reduce over the packed nnz blocks completes the sum.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ba_types.h"
#include "ba_launch.h"
#include "ba_math.h"

// per landmark: Dinv = (Hll + lambda I)^-1, db = Dinv b_l, Y_e = Hpl_e Dinv for its edges
__global__ __launch_bounds__(256) void k_sp_dinv(BaDev D, double lambda)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= D.L) return;
    double Dm[9], Di[9];
    for (int i = 0; i < 9; i++) Dm[i] = D.Hll[9 * (long long)l + i];
    Dm[0] += lambda; Dm[4] += lambda; Dm[8] += lambda;
    ba_inv3(Dm, Di);
    for (int i = 0; i < 9; i++) D.Dinv[9 * (long long)l + i] = Di[i];
    const double b0 = D.bl[3 * (long long)l], b1 = D.bl[3 * (long long)l + 1], b2 = D.bl[3 * (long long)l + 2];
    D.db[3 * (long long)l] = Di[0] * b0 + Di[1] * b1 + Di[2] * b2;
    D.db[3 * (long long)l + 1] = Di[3] * b0 + Di[4] * b1 + Di[5] * b2;
    D.db[3 * (long long)l + 2] = Di[6] * b0 + Di[7] * b1 + Di[8] * b2;
}
// per edge: Y_e = Hpl_e Dinv(landmark of e)  (one thread per edge: nine times the parallelism of a loop inside k_sp_dinv)
// Z_e = Hpl_e L^-T  (6 x 3) with Hll + lambda I = L L^T (Cholesky of the landmark's damped 3 x 3 block): Dinv = L^-T L^-1, so
// Hpl_a Dinv Hpl_b^T = Z_a Z_b^T, and BOTH operands of the Schur GEMM come from this one array.  With Y = Hpl Dinv on one side and
// Hpl on the other the kernel gathered from two arrays of 260 MB each at config 5 -- more than the 256 MB MALL holds; one array
// halves the working set.  (The factor is taken of the block itself, not of its computed inverse: three square roots of pivots that
// are positive whenever the block is.)
__global__ __launch_bounds__(256) void k_sp_edge_y(BaDev D, double lambda)
{
    // The workgroup's 256 blocks of Z (144 bytes each) and of ce (48) lie side by side: passed through LDS and stored as full lines
    // instead of 16 bytes per lane at a stride of 144 (182 -> 112 us at config 5; the same remedy as lm_store_group in ba_kernels.hip).
    __shared__ double2 stage[256 * 9];
    const long long e0 = blockIdx.x * 256LL;
    const long long e = e0 + threadIdx.x;
    double zz[18], cc[6];
    if (e < D.E) {
        const int l = D.edge_point[e];
        double f[6], Bx[18];
        ba_chol3(D.Hll + 9 * (long long)l, lambda, f);               // (pivot guard: see ba_math.h)
        const double2* B = reinterpret_cast<const double2*>(D.Hpl + 18 * e);
#pragma unroll
        for (int i = 0; i < 9; i++) { const double2 v = B[i]; Bx[2 * i] = v.x; Bx[2 * i + 1] = v.y; }
        const double* d = D.db + 3 * (long long)l;
        const double dd[3] = { d[0], d[1], d[2] };
        ba_edge_z_c(Bx, f, dd, zz, cc);
#pragma unroll
        for (int i = 0; i < 9; i++) stage[9 * threadIdx.x + i] = make_double2(zz[2 * i], zz[2 * i + 1]);
    }
    __syncthreads();
    const int ne = (int)min(256LL, D.E - e0);
    double2* zo = reinterpret_cast<double2*>(D.Z + 18 * e0);
#pragma unroll
    for (int j = 0; j < 9; j++) { const int q = j * 256 + threadIdx.x; if (q < 9 * ne) zo[q] = stage[q]; }
    __syncthreads();
    if (e < D.E) {
#pragma unroll
        for (int i = 0; i < 3; i++) stage[3 * threadIdx.x + i] = make_double2(cc[2 * i], cc[2 * i + 1]);
    }
    __syncthreads();
    double2* co = reinterpret_cast<double2*>(D.ce + 6 * e0);
#pragma unroll
    for (int j = 0; j < 3; j++) { const int q = j * 256 + threadIdx.x; if (q < 3 * ne) co[q] = stage[q]; }
}
void sp_launch_dinv(hipStream_t s, const BaDev& D, double lambda)
{
    if (D.L > 0) hipLaunchKernelGGL(k_sp_dinv, dim3(nblk(D.L, 256)), dim3(256), 0, s, D, lambda);
    if (D.E > 0) hipLaunchKernelGGL(k_sp_edge_y, dim3(nblk(D.E, 256)), dim3(256), 0, s, D, lambda);
}

// One workgroup per reduced-camera block: block = Hpp(diag) - sum over its sorted (landmark, pose pair) list of Z_a Z_b^T
// with Z_e = Hpl_e L^-T, Hll + lambda I = L L^T (6x3, k_sp_edge_y; the argument Y is that array).  The sum over pairs is one GEMM with K = 3 x pairs:
// [Y_a1 Y_a2 ...] (6 x K) times [W_b1 W_b2 ...]^T (K x 6), run on the f64 matrix cores as v_mfma_f64_16x16x4_f64
// (M = N = 16 of which 6 are used, K = 4 per instruction: lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15]).
// Four pairs = twelve k = three MFMAs per step (eight pairs per step measured slower); each lane gathers exactly the operand
// elements its (row, k) needs, so the operands never go through LDS.  The four waves of the workgroup take every fourth step
// (a keyframe's diagonal block has as many pairs as the keyframe has observations: one wave per block left a 0.5 ms tail),
// and a wave requests the pair indices two steps and the operands one step ahead of the MFMAs that use them (a step used to
// cost two dependent memory round trips).  The accumulation order -- the hardware's k order inside a wave, wave 0..3 at the
// end -- is fixed: reproducible run to run.
typedef double sp_v4d __attribute__((ext_vector_type(4)));
#define SP_XCD_CHUNK 64         // block pairs per chunk of the chunk-cyclic work order (measured: sp_launch_schur_blocks)
template <int NWV>
__global__ __launch_bounds__(64 * NWV) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_sp_schur_blocks(BaDev D, const double* __restrict__ Y, const unsigned long long* __restrict__ pairs,
                                                         const int* __restrict__ seg_start, const int* __restrict__ seg_end,
                                                         const int* __restrict__ blk_row, const int* __restrict__ blk_col, int nb,
                                                         double* __restrict__ Hb, int per_xcd)
{
    // Workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  The blocks are sorted by (row, column): in dispatch order
    // the ~57 blocks of a block row -- which all gather the row keyframe's Z blocks, and whose column keyframes are the next row's too --
    // are spread over all eight L2s, and every one of them fetches the same operands from the fabric.  per_xcd < 0 (shipped:
    // -SP_XCD_CHUNK): chunks of -per_xcd consecutive block pairs go to one XCD, chunk c to XCD c % 8; per_xcd == 0: dispatch order
    // (sp_launch_schur_blocks has the measurements).
    int wg = (int)blockIdx.x;
    if (per_xcd < 0) {                                  // chunk-cyclic: -per_xcd consecutive block pairs to one XCD
        const int C = -per_xcd, xcd = (int)blockIdx.x & 7, j = (int)blockIdx.x >> 3;
        wg = ((j / C) * 8 + xcd) * C + j % C;
    }
    // TWO reduced blocks per workgroup share the 16 x 16 tile of the MFMA: operand rows 0..5 belong to block 2 g, rows 8..13 to block
    // 2 g + 1 (each with its own pair list), and the tile's two diagonal 6 x 6 corners are the two sums (the off-diagonal corners mix the
    // blocks and are dropped).  The same number of gather loads now serves two blocks: 48 of 64 lanes load instead of 24.
    __shared__ double part[NWV][72];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i16 = lane & 15, kq = lane >> 4;              // operand row of the tile, k within an MFMA
    const int half = i16 >> 3, i = i16 & 7;                 // which of the two blocks, row inside it (< 6 used)
    const int b = 2 * wg + half;
    const bool live = i < 6 && b < nb;
    const int p0 = live ? seg_start[b] : 0, p1 = live ? seg_end[b] : 0;
    // the longer of the workgroup's two lists sets the trip count (wave-uniform)
    int pmax = p1 - p0;
    for (int st = 32; st >= 1; st >>= 1) pmax = max(pmax, __shfl_xor(pmax, st, 64));
    sp_v4d acc = { 0.0, 0.0, 0.0, 0.0 };
    // The twelve k of a step: k = 4 m + kq is column m of pair kq -- a lane's three operand elements are one row of ONE pair's block:
    // one pair index and 24 contiguous bytes per operand (a dwordx4 and a dwordx2), instead of three indices and three scattered
    // doubles.  The kernel's rate is set by its gather requests: 5 loads per step instead of 9.
    const unsigned long long NONE = ~0ull;
    typedef double sp_d2u __attribute__((ext_vector_type(2), aligned(8)));
    auto ld_idx = [&](int q) -> unsigned long long { return (live && p0 + q + kq < p1) ? pairs[p0 + q + kq] : NONE; };   // q = offset into the list
    auto ld_ops = [&](unsigned long long pr, double (&av)[3], double (&bv)[3]) {
        av[0] = av[1] = av[2] = 0.0; bv[0] = bv[1] = bv[2] = 0.0;
        if (pr != NONE) {
            const double* za = Y + 18 * (long long)(unsigned)(pr >> 32) + 3 * i;
            const double* zb = Y + 18 * (long long)(unsigned)(pr & 0xFFFFFFFFu) + 3 * i;
            const sp_d2u a01 = *reinterpret_cast<const sp_d2u*>(za), b01 = *reinterpret_cast<const sp_d2u*>(zb);
            av[0] = a01.x; av[1] = a01.y; av[2] = za[2];
            bv[0] = b01.x; bv[1] = b01.y; bv[2] = zb[2];
        }
    };
    unsigned long long pr_next, pr_far;
    double av[3], bv[3], av_next[3], bv_next[3];
    int q = 4 * wv;                                         // this wave's steps: 4 pairs each, 4 NWV pairs apart
    pr_next = ld_idx(q); ld_ops(pr_next, av, bv); pr_next = ld_idx(q + 4 * NWV);
    for (; q < pmax; q += 4 * NWV) {
        ld_ops(pr_next, av_next, bv_next);
        pr_far = ld_idx(q + 8 * NWV);
#pragma unroll
        for (int m = 0; m < 3; m++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], bv[m], acc, 0, 0, 0);
#pragma unroll
        for (int m = 0; m < 3; m++) { av[m] = av_next[m]; bv[m] = bv_next[m]; }
        pr_next = pr_far;
    }
    // C/D: column = lane & 15, row = (lane >> 4) + 4 * reg; block `half` sits in rows and columns 8 half .. 8 half + 5
    const int c = i16 & 7;
    if (c < 6) {
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = kq + 4 * reg;
            if ((row >> 3) == half && (row & 7) < 6) part[wv][36 * half + 6 * (row & 7) + c] = acc[reg];
        }
    }
    __syncthreads();
    if (threadIdx.x < 72) {
        const int h2 = threadIdx.x / 36, e = threadIdx.x - 36 * h2, bb = 2 * wg + h2;
        if (bb < nb) {
            const int rb = blk_row[bb], cb = blk_col[bb];
            const double base = rb == cb ? D.Hpp[36 * (long long)rb + e] : 0.0;
            double tot = part[0][threadIdx.x];
#pragma unroll
            for (int w2 = 1; w2 < NWV; w2++) tot += part[w2][threadIdx.x];                              // wave 0 .. NWV-1: fixed order
            Hb[36 * (long long)bb + e] = base - tot;
        }
    }
}
void sp_launch_schur_blocks(hipStream_t s, const BaDev& D, const double* Y, const unsigned long long* pairs, const int* st, const int* en,
                            const int* br, const int* bc, int nb, double* Hb)
{
    // few blocks with long pair lists (a local BA: 210 blocks of ~1000 pairs) get 16 waves per block, maps with many blocks 4
    if (nb <= 0) return;
    // measured (config 5, Schur phase of optimize(20), tools/bench_gba.py): dispatch order 4.67 ms, contiguous eighths 8.73 (each XCD then
    // works on a handful of rows at a time and their operands sit in a few L2 channels), chunks of 4 / 16 / 64 / 512 block pairs
    // 4.53 / 4.14 / 4.00 / 4.36 -- 64 ships
    const int nwg = (nb + 1) / 2, grid = (nwg + 8 * SP_XCD_CHUNK - 1) / (8 * SP_XCD_CHUNK) * (8 * SP_XCD_CHUNK);
    if (nb < 2048) hipLaunchKernelGGL(k_sp_schur_blocks<16>, dim3(nwg), dim3(1024), 0, s, D, Y, pairs, st, en, br, bc, nb, Hb, 0);
    else hipLaunchKernelGGL(k_sp_schur_blocks<4>, dim3(grid), dim3(256), 0, s, D, Y, pairs, st, en, br, bc, nb, Hb, -SP_XCD_CHUNK);
}

// one workgroup (4 waves) per free pose: bs = bp - sum over its edges of Hpl_e db(l_e); wave partials added 0..3 (fixed order)
template <int NW>
__global__ __launch_bounds__(64 * NW) void k_sp_bschur(BaDev D, double* __restrict__ bs)
{
    __shared__ double part[NW][6];
    const int f = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (f >= D.nfree) return;
    double c[6] = { 0, 0, 0, 0, 0, 0 };
    for (int k = D.pose_first[f] + threadIdx.x; k < D.pose_first[f + 1]; k += 64 * NW) {
        const double* ce = D.ce + 6 * (long long)D.pose_edges[k];         // Hpl_e db(l_e), left by k_sp_edge_y / the fused linearisation (0 for a dropped edge)
        for (int i = 0; i < 6; i++) c[i] += ce[i];
    }
    for (int i = 0; i < 6; i++)
        for (int s = 32; s >= 1; s >>= 1) c[i] += __shfl_xor(c[i], s, 64);
    if (lane == 0) for (int i = 0; i < 6; i++) part[wv][i] = c[i];
    __syncthreads();
    if (threadIdx.x < 6) {
        double v = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
#pragma unroll
        for (int w = 4; w < NW; w++) v += part[w][threadIdx.x];                                          // wave 0 .. NW-1: fixed order
        bs[6 * (long long)f + threadIdx.x] = D.bp[6 * (long long)f + threadIdx.x] - v;
    }
}

// one wave per free pose: bs = bp - sum over its edges of Hpl_e db(l_e), fixed order
__global__ __launch_bounds__(256) void k_sp_bschur_wave(BaDev D, double* __restrict__ bs)
{
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (f >= D.nfree) return;
    double c[6] = { 0, 0, 0, 0, 0, 0 };
    // four edges in flight per lane: the 48-byte rows are gathered through the keyframe's edge list
    const int k1 = D.pose_first[f + 1];
    for (int k = D.pose_first[f] + lane; k < k1; k += 256) {
        typedef double bs_d2 __attribute__((ext_vector_type(2)));
        bs_d2 v[4][3];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int kk = k + 64 * q;
#pragma unroll
            for (int i = 0; i < 3; i++) v[q][i] = bs_d2{0.0, 0.0};
            if (kk < k1) {
                const bs_d2* ce = reinterpret_cast<const bs_d2*>(D.ce + 6 * (long long)D.pose_edges[kk]);
                v[q][0] = ce[0]; v[q][1] = ce[1]; v[q][2] = ce[2];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) { c[0] += v[q][0].x; c[1] += v[q][0].y; c[2] += v[q][1].x; c[3] += v[q][1].y; c[4] += v[q][2].x; c[5] += v[q][2].y; }
    }
    for (int i = 0; i < 6; i++)
        for (int s = 32; s >= 1; s >>= 1) c[i] += __shfl_xor(c[i], s, 64);
    if (lane < 6) bs[6 * (long long)f + lane] = D.bp[6 * (long long)f + lane] - c[lane];
}
void sp_launch_bschur(hipStream_t s, const BaDev& D, double* bs)
{
    if (D.nfree > 0 && D.nfree < 64) hipLaunchKernelGGL(k_sp_bschur<16>, dim3(D.nfree), dim3(1024), 0, s, D, bs);
    else if (D.nfree > 0 && D.nfree < 512) hipLaunchKernelGGL(k_sp_bschur<4>, dim3(D.nfree), dim3(256), 0, s, D, bs);
    else if (D.nfree > 0) hipLaunchKernelGGL(k_sp_bschur_wave, dim3(nblk(D.nfree, 4)), dim3(256), 0, s, D, bs);
}

__global__ __launch_bounds__(256) void k_sp_add_lambda(const int* __restrict__ diag_id, int nfree, double lambda, double* __restrict__ Hb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nfree * 6) return;
    const int f = i / 6, r = i - 6 * f;
    Hb[36 * (long long)diag_id[f] + 7 * r] += lambda;
}
void sp_launch_add_lambda(hipStream_t s, const int* diag, int nfree, double lambda, double* Hb)
{ hipLaunchKernelGGL(k_sp_add_lambda, dim3(nblk(6LL * nfree, 256)), dim3(256), 0, s, diag, nfree, lambda, Hb); }

// packed blocks -> dense row-major n x n (upper block triangle), for the dense path
__global__ __launch_bounds__(256) void k_sp_to_dense(const double* __restrict__ Hb, const int* __restrict__ blk_row, const int* __restrict__ blk_col,
                                                     int nb, long long n, double* __restrict__ Hs)
{
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= 36LL * nb) return;
    const int b = (int)(i / 36), e = (int)(i - 36LL * b), r = e / 6, c = e - 6 * r;
    Hs[(6LL * blk_row[b] + r) * n + 6 * blk_col[b] + c] = Hb[i];
}
void sp_launch_to_dense(hipStream_t s, const double* Hb, const int* br, const int* bc, int nb, long long n, double* Hs)
{ hipLaunchKernelGGL(k_sp_to_dense, dim3(nblk(36LL * nb, 256)), dim3(256), 0, s, Hb, br, bc, nb, n, Hs); }
