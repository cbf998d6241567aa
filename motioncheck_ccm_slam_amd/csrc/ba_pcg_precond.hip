// ba_pcg_precond.hip -- the two levels of the PCG's preconditioner, built once per LM trial and applied by the iterations
// (ba_pcg.hip, ba_ppcg.hip): cluster inverses and the coarse matrix Ac = P^T H P (inverted by ba_dense.hip's dense_launch_invert).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ba_types.h"
#include "ba_launch.h"
#include "ba_pcg.h"

// ---------------------------------------------------------------------------------------- cluster level
// Cluster-Jacobi preconditioner: M = the diagonal blocks of PCG_CL consecutive free keyframes INCLUDING the coupling
// blocks between them (consecutive keyframes of a trajectory share most of their landmarks, so these are the strongest
// off-diagonal blocks of the reduced camera system); its inverse is a dense PCG_CN x PCG_CN matrix per cluster, applied
// as a mat-vec.  Minv layout: [cluster][PCG_CN][PCG_CN], symmetric.
__global__ __launch_bounds__(256) void k_pcg_cl_gather(const double* __restrict__ Hb, const int* __restrict__ blk_row, const int* __restrict__ blk_col,
                                                       int nb, double* __restrict__ Mc)
{
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= 36LL * nb) return;
    const int b = (int)(i / 36), e = (int)(i - 36LL * b), r = e / 6, c = e - 6 * r;
    const int br = blk_row[b], bc = blk_col[b];
    if (br / PCG_CL != bc / PCG_CL) return;
    double* M = Mc + (long long)(br / PCG_CL) * PCG_CN * PCG_CN;
    const int rr = 6 * (br % PCG_CL) + r, cc = 6 * (bc % PCG_CL) + c;
    const double v = Hb[i];
    // The upper block triangle is stored once, so an off-diagonal block is mirrored.  Of a diagonal block only the upper
    // half is used, mirrored as well: taking both halves would let two not-quite-equal values race into one slot (seen
    // as 1e-15 run-to-run noise) and leave the preconditioner not exactly symmetric.
    if (br == bc && r > c) return;
    M[rr * PCG_CN + cc] = v;
    M[cc * PCG_CN + rr] = v;
}
// in-place inverse of every cluster matrix by Gauss-Jordan without pivoting (SPD); unused rows of the last cluster
// are made identity; a non-positive pivot raises `bad`.  The matrix lives in REGISTERS: thread (ty, tx) of the 16 x 16 workgroup owns
// the 3 x 3 elements (ty + 16 a, tx + 16 b); per pivot p the owners of column p and of row p publish them in LDS (two alternating
// buffers: one barrier per pivot) and every thread reads the three column and three row values its elements need -- the scheme of
// k_inv_diag in ba_dense.hip.  (Round 2 held the matrix in LDS with two barriers per pivot: 71 us per LM trial, on the critical path.)
static_assert(PCG_CN == 48, "k_pcg_cl_invert tiles a 48 x 48 cluster as 16 x 16 threads x 3 x 3 elements");
__global__ __launch_bounds__(256) void k_pcg_cl_invert(double* __restrict__ Mc, int nfree, int* __restrict__ bad)
{
    __shared__ double fcol[2][PCG_CN], prow[2][PCG_CN];
    __shared__ int s_bad;
    double* M = Mc + (long long)blockIdx.x * PCG_CN * PCG_CN;
    const int used = 6 * min(PCG_CL, nfree - (int)blockIdx.x * PCG_CL);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double a[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { const int r = ty + 16 * i, c = tx + 16 * j; a[i][j] = (r < used && c < used) ? M[r * PCG_CN + c] : (r == c ? 1.0 : 0.0); }
    if (threadIdx.x == 0) s_bad = 0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            if (tx + 16 * j == 0) fcol[0][ty + 16 * i] = a[i][j];
            if (ty + 16 * i == 0) prow[0][tx + 16 * j] = a[i][j];
        }
    __syncthreads();
    for (int p = 0; p < PCG_CN; p++) {
        const int cur = p & 1, nxt = cur ^ 1;
        const double piv = prow[cur][p];
        if (!(piv > 0.0) && threadIdx.x == 0) s_bad = 1;
        const double ip = 1.0 / piv;
        double fc[3], pr[3];
#pragma unroll
        for (int i = 0; i < 3; i++) fc[i] = fcol[cur][ty + 16 * i];
#pragma unroll
        for (int j = 0; j < 3; j++) { const int c = tx + 16 * j; pr[j] = (c == p ? 1.0 : prow[cur][c]) * ip; }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int r = ty + 16 * i, c = tx + 16 * j;
                a[i][j] = r == p ? pr[j] : ((c == p ? 0.0 : a[i][j]) - fc[i] * pr[j]);
                if (c == p + 1) fcol[nxt][r] = a[i][j];
                if (r == p + 1) prow[nxt][c] = a[i][j];
            }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[(ty + 16 * i) * PCG_CN + tx + 16 * j] = a[i][j];
    if (threadIdx.x == 0 && s_bad) atomicOr(bad, 1);
}
size_t pcg_minv_bytes(int nfree) { return (size_t)nblk(nfree, PCG_CL) * PCG_CN * PCG_CN * 8; }
hipError_t pcg_launch_minv(hipStream_t s, const double* Hb, const int* blk_row, const int* blk_col, int nb, int nfree, double* Minv, int* bad)
{
    const int ncl = nblk(nfree, PCG_CL);
    hipError_t e = hipMemsetAsync(Minv, 0, pcg_minv_bytes(nfree), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_pcg_cl_gather, dim3(nblk(36LL * nb, 256)), dim3(256), 0, s, Hb, blk_row, blk_col, nb, Minv);
    hipLaunchKernelGGL(k_pcg_cl_invert, dim3(ncl), dim3(256), 0, s, Minv, nfree, bad);
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------- coarse level
// Second level of the preconditioner (additive two-level Schwarz): the cluster inverses above damp the error inside a
// cluster, but the slowly varying error along the trajectory (many keyframes drifting together) converges only as fast as
// information travels from cluster to cluster.  Coarse space, 7 unknowns per aggregate of A = PCG_CL * pcg_agg_clusters()
// keyframes: a rigid increment (6) and a scale change about the aggregate's centre (a monocular map with one fixed keyframe
// has a free scale; its local version is the softest deformation of a trajectory piece), interpolated LINEARLY between the
// aggregate centres (hat functions: keyframe f takes 1 - a of aggregate I and a of I + 1, x = (f + 1/2) / A - 1/2 = I + a;
// the ends are clamped).  P = prolongation (n x 7 nagg), Ac = P^T H P dense and small, inverted once per LM trial (block
// Gauss-Jordan of ba_dense.hip), and      z = Minv r + P Ac^-1 P^T r.
// Iterations of a late LM trial of config 5 (lambda = 0.04, relative residual 1e-6; tools/gba_coarse_study.py reproduces the
// counts on the CPU): cluster level alone 1165, piecewise-constant rigid aggregates (round 2 until here) 517, hat functions 148,
// hat functions + scale 98.
// (PCG_AGG, pcg_agg_clusters, pcg_hat, pcg_hat_weight, pcg_hat_support: ba_pcg.h)
// coarse level: sizes, set-up (Ac into `Ac`, upper triangle row-major; the caller factors and inverts it, then mirrors)
int pcg_coarse_aggregates(int nfree) { return nblk(nfree, PCG_CL * pcg_agg_clusters(nfree)); }
int pcg_coarse_agg_keyframes(int nfree) { return PCG_CL * pcg_agg_clusters(nfree); }
int pcg_coarse_dim(int nfree) { return PCG_CDOF * pcg_coarse_aggregates(nfree); }
int pcg_coarse_pitch(int nfree) { return dense_pitch(pcg_coarse_dim(nfree)); }
int pcg_coarse_parts(int nfree) { return nblk(pcg_coarse_dim(nfree), 4); }
// upper triangle of Ac = P^T H P, row-major with pitch ncp: one workgroup per aggregate pair I <= J, thread = keyframe pair
// (i, j) of the two supports, the 49 sums reduced over the workgroup in a fixed order (the ranks of a sharded solve must get
// the same bits).  Column 6 of keyframe i's 6 x 7 basis W_i is (0, 0, 0, t_i - c_I): svec holds t_i, cen the aggregate centres.
// (the grid runs over the aggregate pairs that hold at least one block -- `pairs`, made once per call by k_pcg_coarse_mark and the
// host: 1 in 8 of the upper triangle at config 5; as a full nagg x nagg grid the kernel flooded the chip from the side stream for
// 0.26 ms per trial, and the PCG's 1024-thread workgroups starved behind its small ones)
__global__ __launch_bounds__(256) void k_pcg_coarse_mark(const int* __restrict__ blk_row, const int* __restrict__ blk_col, int nb, int nfree, int nagg, uint8_t* __restrict__ aggmap)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    const int A = PCG_CL * pcg_agg_clusters(nfree);
    const PcgHat ha = pcg_hat(blk_row[i], A, nagg), hb = pcg_hat(blk_col[i], A, nagg);
    const int ia[2] = { ha.i0, ha.i1 }, ib[2] = { hb.i0, hb.i1 };
    for (int x = 0; x < 2; x++)
        for (int y = 0; y < 2; y++) aggmap[min(ia[x], ib[y]) * nagg + max(ia[x], ib[y])] = 1;
}
void pcg_launch_coarse_mark(hipStream_t s, const int* blk_row, const int* blk_col, int nb, int nfree, uint8_t* aggmap)
{
    if (nb > 0) hipLaunchKernelGGL(k_pcg_coarse_mark, dim3(nblk(nb, 256)), dim3(256), 0, s, blk_row, blk_col, nb, nfree, pcg_coarse_aggregates(nfree), aggmap);
}
__global__ __launch_bounds__(256) void k_pcg_coarse_build(const double* __restrict__ Hb, const uint8_t* __restrict__ map, const int* __restrict__ id,
                                                          int nfree, int nagg, int ncp, const double* __restrict__ svec, const double* __restrict__ cen,
                                                          const int* __restrict__ pairs, double* __restrict__ Ac)
{
    __shared__ double red[4][PCG_CDOF * PCG_CDOF];
    const int I = pairs[2 * blockIdx.x], J = pairs[2 * blockIdx.x + 1];
    if (J < I) return;
    const int A = PCG_CL * pcg_agg_clusters(nfree);
    int i0, i1, j0, j1;
    pcg_hat_support(I, A, nfree, i0, i1); pcg_hat_support(J, A, nfree, j0, j1);
    const int ni = i1 - i0, nj = j1 - j0;
    double acc[PCG_CDOF * PCG_CDOF];
#pragma unroll
    for (int e = 0; e < PCG_CDOF * PCG_CDOF; e++) acc[e] = 0.0;
    for (int t = threadIdx.x; t < ni * nj; t += 256) {
        const int i = i0 + t / nj, j = j0 + t % nj;
        const int a = min(i, j), b = max(i, j);
        const long long idx = (long long)a * nfree + b;
        if (!map[idx]) continue;
        const double wij = pcg_hat_weight(i, I, A, nagg) * pcg_hat_weight(j, J, A, nagg);
        if (wij == 0.0) continue;
        const double* B = Hb + 36LL * id[idx];
        double si[3], sj[3];
#pragma unroll
        for (int q = 0; q < 3; q++) { si[q] = svec[3 * i + q] - cen[3 * I + q]; sj[q] = svec[3 * j + q] - cen[3 * J + q]; }
        double col6[6], row6[6] = { 0, 0, 0, 0, 0, 0 }, corner = 0.0;
#pragma unroll
        for (int d = 0; d < 6; d++) {
            double c6 = 0.0;
#pragma unroll
            for (int e = 0; e < 6; e++) {
                // block (a, b) is stored for a <= b; (i, j) with i > j is its transpose; of a diagonal block the upper half counts
                const double v = i < j ? B[6 * d + e] : (i > j ? B[6 * e + d] : (d <= e ? B[6 * d + e] : B[6 * e + d]));
                acc[PCG_CDOF * d + e] += wij * v;
                if (e >= 3) c6 += v * sj[e - 3];
                if (d >= 3) row6[e] += si[d - 3] * v;
            }
            col6[d] = c6;
            if (d >= 3) corner += si[d - 3] * c6;
        }
#pragma unroll
        for (int d = 0; d < 6; d++) { acc[PCG_CDOF * d + 6] += wij * col6[d]; acc[PCG_CDOF * 6 + d] += wij * row6[d]; }
        acc[PCG_CDOF * 6 + 6] += wij * corner;
    }
#pragma unroll
    for (int e = 0; e < PCG_CDOF * PCG_CDOF; e++) {
        double v = acc[e];
        for (int st = 32; st >= 1; st >>= 1) v += __shfl_xor(v, st, 64);
        acc[e] = v;
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int e = 0; e < PCG_CDOF * PCG_CDOF; e++) red[threadIdx.x >> 6][e] = acc[e];
    }
    __syncthreads();
    if (threadIdx.x < PCG_CDOF * PCG_CDOF) {
        const int d = threadIdx.x / PCG_CDOF, e = threadIdx.x - PCG_CDOF * d;
        const int r = PCG_CDOF * I + d, c = PCG_CDOF * J + e;
        if (r <= c) Ac[(long long)r * ncp + c] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    }
}
// Ac was built as an upper triangle: make it the full ncp x ncp matrix the inversion works on (lower from upper, identity
// in the padding beyond nc)
__global__ __launch_bounds__(256) void k_pcg_coarse_complete(double* __restrict__ A, int nc, int ncp)
{
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= (long long)ncp * ncp) return;
    const int r = (int)(i / ncp), c = (int)(i - (long long)r * ncp);
    if (r >= nc || c >= nc) A[i] = r == c ? 1.0 : 0.0;
    else if (r > c) A[i] = A[(long long)c * ncp + r];
    else if (r == c && A[i] == 0.0) A[i] = 1.0;      // an aggregate whose keyframes all sit at one point has no scale column: the unknown stays inert
}
// (dense_launch_solve in ba_dense.hip completes the reduced system of a small map with it too)
void pcg_launch_coarse_complete(hipStream_t s, double* A, int nc, int ncp)
{
    hipLaunchKernelGGL(k_pcg_coarse_complete, dim3(nblk((long long)ncp * ncp, 256)), dim3(256), 0, s, A, nc, ncp);
}
// Ac = P^T H P as a full (padded) matrix in `Ac`
hipError_t pcg_launch_coarse_build(hipStream_t s, const double* Hb, const uint8_t* map, const int* id, int nfree, const double* svec, const double* cen,
                                   const int* pairs, int npairs, double* Ac)
{
    const int nagg = pcg_coarse_aggregates(nfree), nc = PCG_CDOF * nagg, ncp = pcg_coarse_pitch(nfree);
    hipError_t e = hipMemsetAsync(Ac, 0, (size_t)ncp * ncp * sizeof(double), s);          // aggregate pairs without a block stay zero
    if (e != hipSuccess) return e;
    if (npairs > 0) hipLaunchKernelGGL(k_pcg_coarse_build, dim3(npairs), dim3(256), 0, s, Hb, map, id, nfree, nagg, ncp, svec, cen, pairs, Ac);
    pcg_launch_coarse_complete(s, Ac, nc, ncp);
    return hipSuccess;
}
// after the inversion: the upper triangle is mirrored so that the preconditioner is exactly symmetric
__global__ __launch_bounds__(256) void k_pcg_coarse_mirror(double* __restrict__ A, int ncp)
{
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= (long long)ncp * ncp) return;
    const int r = (int)(i / ncp), c = (int)(i - (long long)r * ncp);
    if (r > c) A[i] = A[(long long)c * ncp + r];
}
void pcg_launch_coarse_mirror(hipStream_t s, double* A, int ncp)
{
    hipLaunchKernelGGL(k_pcg_coarse_mirror, dim3(nblk((long long)ncp * ncp, 256)), dim3(256), 0, s, A, ncp);
}
