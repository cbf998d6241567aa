// ba_dense.hip -- the two dense solvers of the reduced camera system (small maps; fallback of the PCG) and the in-place inverse
// of a symmetric positive definite matrix that the PCG's coarse level uses too.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ba_types.h"
#include "ba_launch.h"

// Reduced systems of a local BA (config 4: 20 free keyframes, n = 120 unknowns) are solved by ONE workgroup in one launch: L L^T
// factorisation and both triangular solves.  The block Gauss-Jordan path below needs ~14 launches for such a system and took
// 0.5 ms per LM trial -- 70 % of the whole local BA.  n <= DENSE_SMALL_MAX so that every tile of the lower triangle has its thread.
#define DENSE_SMALL_MAX 138
#define DS_TPB 576
// Every 6x6 tile of the lower triangle lives in the REGISTERS of TWO neighbouring threads for the whole solve, three rows each
// (n <= 138: at most 276 tiles, 552 threads): per block column the diagonal tile's owners factor it and publish it in LDS, the owners
// of the tiles below solve against it (multiplying by the reciprocals of its diagonal: a double-precision division is ~12
// instructions, 36 of them per tile and column were a fifth of the kernel) and publish the panel, every remaining tile subtracts
// panel_I panel_K^T from its registers -- two barriers per block column, and the only LDS traffic is the panel and the right-hand
// side.  The forward substitution rides along with the factorisation and the backward one reads the factor from the registers it
// already is in, so the factor is never written anywhere.  (History at n = 120: matrix in LDS column by column 256 us, blocked in LDS
// 133 us, register tiles + the factor copied to LDS for two separate substitution loops 116 us, one thread per tile 88 us: the
// kernel is bound by the double-precision instructions its busiest thread issues per block column -- 216 multiply-adds of a trailing
// tile, now 108 -- not by anything a second workgroup could share.)  The two owners of a diagonal tile exchange their rows by
// shuffles and BOTH run the serial 6 x 6 factorisation, so neither waits for the other's result.
// The damping is added to the diagonal while the tiles are loaded and the verdict is WRITTEN (0 / 1) rather than or-ed in: the
// launches of k_sp_add_lambda and of the memset of `bad` in front of this kernel were two of a local BA trial's thirteen.
__global__ __launch_bounds__(DS_TPB) void k_dense_small_solve(const double* __restrict__ Hb, const int* __restrict__ blk_row, const int* __restrict__ blk_col,
                                                              int nb, int n, const double* __restrict__ b, double* __restrict__ x, int* __restrict__ bad, double lambda)
{
    extern __shared__ double ds_lds[];
    double* v = ds_lds;                      // [n] right-hand side -> y -> solution
    __shared__ double s_ljj[36], s_linv[6], s_y[6];
    __shared__ double s_panel[DENSE_SMALL_MAX / 6][36];
    __shared__ int s_tile_blk[DENSE_SMALL_MAX / 6 * (DENSE_SMALL_MAX / 6 + 1) / 2];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int nbk = n / 6, ntiles = nbk * (nbk + 1) / 2;
    if (tid == 0) s_bad = 0;
    for (int i = tid; i < ntiles; i += DS_TPB) s_tile_blk[i] = -1;
    for (int i = tid; i < n; i += DS_TPB) v[i] = b[i];
    __syncthreads();
    for (int k = tid; k < nb; k += DS_TPB) { const int r = blk_row[k], c = blk_col[k]; if (r <= c && c < nbk) s_tile_blk[c * (c + 1) / 2 + r] = k; }
    __syncthreads();
    // rows 3 p .. 3 p + 2 of tile (I, K), K <= I
    const int tile = tid >> 1, p = tid & 1;
    int I = 0, K = 0;
    const bool have = tile < ntiles;
    // tiles in COLUMN-major order (block column K, then block row I): the tiles still at work in step J -- K >= J -- are the tail of
    // the thread range, so the waves in front of it skip a step's phases altogether instead of issuing them for one or two live lanes
    // (row-major order kept every wave busy until the last columns: 79.6 against 68.2 us at n = 120)
    if (have) { int t = tile; while (t >= nbk - K) { t -= nbk - K; K++; } I = K + t; }
    const int tile_rm = I * (I + 1) / 2 + K;                                 // its index in s_tile_blk (row-major)
    double T[3][6];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 6; k++) T[i][k] = 0.0;
    if (have && s_tile_blk[tile_rm] >= 0) {
        const double* B = Hb + 36LL * s_tile_blk[tile_rm];                   // stored block (row K, col I): tile(i, k) = B[k][i]
#pragma unroll
        for (int ii = 0; ii < 3; ii++) {
            const int i = 3 * p + ii;
#pragma unroll
            for (int k = 0; k < 6; k++) {
                // a diagonal block is stored whole; keep it exactly symmetric (upper half wins)
                T[ii][k] = (I == K) ? B[max(i, k) * 6 + min(i, k)] : B[k * 6 + i];
                if (I == K && k == i) T[ii][k] += lambda;
            }
        }
    }
    // the full diagonal tile out of its two owners' rows (both owners call this together: they are neighbouring lanes of one wave)
    auto gather_diag = [&](double (&F)[6][6]) {
#pragma unroll
        for (int ii = 0; ii < 3; ii++)
#pragma unroll
            for (int k = 0; k < 6; k++) {
                const double mine = T[ii][k], other = __shfl_xor(mine, 1, 64);
                F[ii][k] = p ? other : mine;
                F[3 + ii][k] = p ? mine : other;
            }
    };
    double dinv[6] = { 0, 0, 0, 0, 0, 0 };                                   // a diagonal tile's owners: 1 / L_cc
    // factorisation, with the forward substitution L y = b riding along: the diagonal tile's owners solve its six unknowns as soon
    // as the tile is factored, and the owner of a panel tile's row takes its product with y_J off b_I when the row is final
    // (one writer per unknown and step).  Two barriers per block column.
    for (int J = 0; J < nbk; J++) {
        const int j0 = 6 * J;
        if (have && I == J && K == J) {                                      // 6x6 Cholesky of the diagonal tile, by both owners alike
            double F[6][6];
            gather_diag(F);
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double d = F[c][c];
#pragma unroll
                for (int k = 0; k < c; k++) d -= F[c][k] * F[c][k];
                if (!(d > 0.0)) { s_bad = 1; d = 1.0; }
                // 1 / sqrt(d) once, sqrt(d) = d / sqrt(d): a square root AND a division per pivot were two ~25-instruction sequences on the
                // threads every other thread waits for (a third of the kernel)
                const double id = rsqrt(d);
                F[c][c] = d * id;
                dinv[c] = id;
#pragma unroll
                for (int r = c + 1; r < 6; r++) {
                    double w = F[r][c];
#pragma unroll
                    for (int k = 0; k < c; k++) w -= F[r][k] * F[c][k];
                    F[r][c] = w * id;
                }
            }
            double y[6];
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double w = v[j0 + c];
#pragma unroll
                for (int k = 0; k < c; k++) w -= F[c][k] * y[k];
                y[c] = w * dinv[c];
            }
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int k = 0; k < 6; k++) if (k > i) F[i][k] = 0.0;
#pragma unroll
            for (int ii = 0; ii < 3; ii++)
#pragma unroll
                for (int k = 0; k < 6; k++) T[ii][k] = p ? F[3 + ii][k] : F[ii][k];
            if (p == 0) {
#pragma unroll
                for (int i = 0; i < 6; i++) {
#pragma unroll
                    for (int k = 0; k < 6; k++) s_ljj[i * 6 + k] = F[i][k];
                    s_linv[i] = dinv[i]; s_y[i] = y[i]; v[j0 + i] = y[i];
                }
            }
        }
        __syncthreads();
        if (have && K == J && I > J) {                                       // panel tile: X L_JJ^T = T, row by row
            double lj[6][6], li[6], yj[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                li[i] = s_linv[i]; yj[i] = s_y[i];
#pragma unroll
                for (int k = 0; k < i; k++) lj[i][k] = s_ljj[i * 6 + k];
            }
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    double w = T[r][c];
#pragma unroll
                    for (int k = 0; k < c; k++) w -= T[r][k] * lj[c][k];
                    T[r][c] = w * li[c];
                }
#pragma unroll
            for (int ii = 0; ii < 3; ii++) {
                const int i = 3 * p + ii;
#pragma unroll
                for (int k = 0; k < 6; k++) s_panel[I][i * 6 + k] = T[ii][k];
                v[6 * I + i] -= ((T[ii][0] * yj[0] + T[ii][1] * yj[1]) + (T[ii][2] * yj[2] + T[ii][3] * yj[3])) + (T[ii][4] * yj[4] + T[ii][5] * yj[5]);
            }
        }
        __syncthreads();
        if (have && K > J) {                                                 // trailing tile: T -= panel_I panel_K^T
            double pi[3][6], pk[6][6];
#pragma unroll
            for (int ii = 0; ii < 3; ii++)
#pragma unroll
                for (int k = 0; k < 6; k++) pi[ii][k] = s_panel[I][(3 * p + ii) * 6 + k];
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int k = 0; k < 6; k++) pk[i][k] = s_panel[K][i * 6 + k];
#pragma unroll
            for (int ii = 0; ii < 3; ii++)
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    double w = 0;
#pragma unroll
                    for (int q = 0; q < 6; q++) w += pi[ii][q] * pk[k][q];
                    T[ii][k] -= w;
                }
        }
    }
    __syncthreads();
    // L^T x = y from the tiles where they are (registers): block row J of L is what column J of L^T needs
    for (int J = nbk - 1; J >= 0; J--) {
        const int j0 = 6 * J;
        if (have && I == J && K == J) {
            double F[6][6], xx[6];
            gather_diag(F);
#pragma unroll
            for (int c = 5; c >= 0; c--) {
                double w = v[j0 + c];
#pragma unroll
                for (int k = c + 1; k < 6; k++) w -= F[k][c] * xx[k];
                xx[c] = w * dinv[c];
            }
            if (p == 0) {
#pragma unroll
                for (int c = 0; c < 6; c++) { v[j0 + c] = xx[c]; s_y[c] = xx[c]; }
            }
        }
        __syncthreads();
        if (have && I == J && K < J) {
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double w = 0;
#pragma unroll
                for (int rr = 0; rr < 3; rr++) w += T[rr][c] * s_y[3 * p + rr];
                w += __shfl_xor(w, 1, 64);                                   // the tile's other three rows
                if (p == 0) v[6 * K + c] -= w;
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += DS_TPB) x[i] = v[i];
    if (tid == 0) *bad = s_bad ? 1 : 0;
}
int dense_small_max() { return DENSE_SMALL_MAX; }
int dense_launch_small_solve(hipStream_t s, const double* Hb, const int* blk_row, const int* blk_col, int nb, int n, const double* b, double* x, int* bad, double lambda)
{
    const size_t lds = (size_t)(n + 8) * sizeof(double);
    if (hipFuncSetAttribute((const void*)k_dense_small_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dense_small_solve, dim3(1), dim3(DS_TPB), lds, s, Hb, blk_row, blk_col, nb, n, b, x, bad, lambda);
    return 0;
}

// ---- dense inverse of a symmetric positive definite matrix (the PCG's coarse matrix; the reduced system of a small map): in-place
// block Gauss-Jordan without pivoting,
// 48 x 48 blocks, four small kernels per block step, every sum in a fixed order -- the result is the same bits on every
// run and every rank (rocSOLVER's potrf + potri, used here first, differed in the last bits from run to run).
//   D = A_kk^-1;  A_kj <- D A_kj (j != k);  A_ij <- A_ij - A_ik A_kj (i, j != k);  A_ik <- -A_ik D (i != k);  A_kk <- D
#define INV_B 48
#define INV_T 3                  // a thread of the 16 x 16 workgroup owns INV_T x INV_T outputs of a block
static_assert(INV_B == 16 * INV_T, "256 threads tile a block");
// D = A_kk^-1 by in-place Gauss-Jordan in LDS
__global__ __launch_bounds__(256) void k_inv_diag(const double* __restrict__ A, int lda, int k, double* __restrict__ D, int* __restrict__ bad)
{
    // Gauss-Jordan with the block in REGISTERS: thread (ty, tx) of the 16 x 16 workgroup owns the 3 x 3 elements (ty + 16 a, tx + 16 b);
    // per pivot p the owners of column p and of row p publish them in LDS (two alternating buffers: one barrier per pivot), every
    // thread reads the three column and three row values its elements need.  (With the block in LDS and two barriers per pivot the
    // 19 diagonal blocks of config 5's coarse matrix took 73 us each -- 60 % of the inversion, which shares the GPU with the PCG.)
    __shared__ double fcol[2][INV_B], prow[2][INV_B];
    __shared__ int s_bad;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const double* Akk = A + ((long long)k * INV_B) * lda + (long long)k * INV_B;
    double a[INV_T][INV_T];
#pragma unroll
    for (int i = 0; i < INV_T; i++)
#pragma unroll
        for (int j = 0; j < INV_T; j++) a[i][j] = Akk[(long long)(ty + 16 * i) * lda + tx + 16 * j];
    if (threadIdx.x == 0) s_bad = 0;
    // publish column 0 and row 0
#pragma unroll
    for (int i = 0; i < INV_T; i++)
#pragma unroll
        for (int j = 0; j < INV_T; j++) {
            if (tx + 16 * j == 0) fcol[0][ty + 16 * i] = a[i][j];
            if (ty + 16 * i == 0) prow[0][tx + 16 * j] = a[i][j];
        }
    __syncthreads();
    for (int p = 0; p < INV_B; p++) {
        const int cur = p & 1, nxt = cur ^ 1;
        const double piv = prow[cur][p];
        if (!(piv > 0.0) && threadIdx.x == 0) s_bad = 1;
        const double ip = 1.0 / piv;
        double fc[INV_T], pr[INV_T];
#pragma unroll
        for (int i = 0; i < INV_T; i++) fc[i] = fcol[cur][ty + 16 * i];
#pragma unroll
        for (int j = 0; j < INV_T; j++) { const int c = tx + 16 * j; pr[j] = (c == p ? 1.0 : prow[cur][c]) * ip; }
#pragma unroll
        for (int i = 0; i < INV_T; i++)
#pragma unroll
            for (int j = 0; j < INV_T; j++) {
                const int r = ty + 16 * i, c = tx + 16 * j;
                a[i][j] = r == p ? pr[j] : ((c == p ? 0.0 : a[i][j]) - fc[i] * pr[j]);
                if (c == p + 1) fcol[nxt][r] = a[i][j];
                if (r == p + 1) prow[nxt][c] = a[i][j];
            }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < INV_T; i++)
#pragma unroll
        for (int j = 0; j < INV_T; j++) D[(ty + 16 * i) * INV_B + tx + 16 * j] = a[i][j];
    if (threadIdx.x == 0 && s_bad) atomicOr(bad, 1);
}
// C (one block, in registers: thread = INV_T x INV_T outputs) = X Y with X, Y staged in LDS; k ascending
__device__ __forceinline__ void inv_mm(const double (*X)[INV_B], const double (*Y)[INV_B], double (&c)[INV_T][INV_T])
{
    const int tr = INV_T * (threadIdx.x >> 4), tc = INV_T * (threadIdx.x & 15);
#pragma unroll
    for (int i = 0; i < INV_T; i++)
#pragma unroll
        for (int j = 0; j < INV_T; j++) c[i][j] = 0.0;
    for (int kk = 0; kk < INV_B; kk++) {
        double x[INV_T], y[INV_T];
#pragma unroll
        for (int i = 0; i < INV_T; i++) { x[i] = X[tr + i][kk]; y[i] = Y[kk][tc + i]; }
#pragma unroll
        for (int i = 0; i < INV_T; i++)
#pragma unroll
            for (int j = 0; j < INV_T; j++) c[i][j] += x[i] * y[j];
    }
}
__device__ __forceinline__ void inv_load(double (*T)[INV_B], const double* __restrict__ src, int ld)
{
    for (int i = threadIdx.x; i < INV_B * INV_B; i += 256) { const int r = i / INV_B, c = i - r * INV_B; T[r][c] = src[(long long)r * ld + c]; }
}
// mode 0: A_kj <- D A_kj (block column j = blockIdx.x, skipping k);  mode 1: A_ik <- -A_ik D (block row i = blockIdx.x, skipping k; the
// extra last workgroup stores A_kk <- D);  mode 2: A_ij <- A_ij - A_ik A_kj (i = blockIdx.y, j = blockIdx.x, both skipping k)
__global__ __launch_bounds__(256) void k_inv_step(double* __restrict__ A, int lda, int nblk, int k, const double* __restrict__ D, int mode)
{
    __shared__ double X[INV_B][INV_B], Y[INV_B][INV_B];
    const int tr = INV_T * (threadIdx.x >> 4), tc = INV_T * (threadIdx.x & 15);
    auto blk = [&](int bi, int bj) { return A + ((long long)bi * INV_B) * lda + (long long)bj * INV_B; };
    double c[INV_T][INV_T];
    if (mode == 1 && (int)blockIdx.x == nblk - 1) {                    // A_kk <- D
        double* K = blk(k, k);
        for (int i = threadIdx.x; i < INV_B * INV_B; i += 256) K[(long long)(i / INV_B) * lda + i % INV_B] = D[i];
        return;
    }
    const int bx = (int)blockIdx.x + ((int)blockIdx.x >= k ? 1 : 0);
    if (mode == 0) {
        double* T = blk(k, bx);
        inv_load(X, D, INV_B); inv_load(Y, T, lda);
        __syncthreads();
        inv_mm(X, Y, c);
#pragma unroll
        for (int i = 0; i < INV_T; i++)
#pragma unroll
            for (int j = 0; j < INV_T; j++) T[(long long)(tr + i) * lda + tc + j] = c[i][j];
    } else if (mode == 1) {
        double* T = blk(bx, k);
        inv_load(X, T, lda); inv_load(Y, D, INV_B);
        __syncthreads();
        inv_mm(X, Y, c);
#pragma unroll
        for (int i = 0; i < INV_T; i++)
#pragma unroll
            for (int j = 0; j < INV_T; j++) T[(long long)(tr + i) * lda + tc + j] = -c[i][j];
    } else {
        const int by = (int)blockIdx.y + ((int)blockIdx.y >= k ? 1 : 0);
        double* T = blk(by, bx);
        inv_load(X, blk(by, k), lda); inv_load(Y, blk(k, bx), lda);
        __syncthreads();
        inv_mm(X, Y, c);
#pragma unroll
        for (int i = 0; i < INV_T; i++)
#pragma unroll
            for (int j = 0; j < INV_T; j++) T[(long long)(tr + i) * lda + tc + j] -= c[i][j];
    }
}
// in-place inverse of the ncp x ncp matrix A (ncp a multiple of INV_B); D = one block of scratch; *bad is raised on a non-positive pivot
void dense_launch_invert(hipStream_t s, double* A, int ncp, double* D, int* bad)
{
    const int nb = ncp / INV_B;
    for (int k = 0; k < nb; k++) {
        hipLaunchKernelGGL(k_inv_diag, dim3(1), dim3(256), 0, s, A, ncp, k, D, bad);
        if (nb > 1) hipLaunchKernelGGL(k_inv_step, dim3(nb - 1), dim3(256), 0, s, A, ncp, nb, k, D, 0);
        if (nb > 1) hipLaunchKernelGGL(k_inv_step, dim3(nb - 1, nb - 1), dim3(256), 0, s, A, ncp, nb, k, D, 2);
        hipLaunchKernelGGL(k_inv_step, dim3(nb), dim3(256), 0, s, A, ncp, nb, k, D, 1);
    }
}

// y = A x for a dense row-major n x n matrix of pitch lda: a wave per row, lanes stride the columns, fixed butterfly
__global__ __launch_bounds__(256) void k_dense_matvec(const double* __restrict__ A, int n, int lda, const double* __restrict__ x, double* __restrict__ y)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const double* a = A + (long long)row * lda;
    double s = 0;
    for (int c = lane; c < n; c += 64) s += a[c] * x[c];
    for (int st = 32; st >= 1; st >>= 1) s += __shfl_xor(s, st, 64);
    if (lane == 0) y[row] = s;
}
int dense_pitch(long long n) { return (int)((n + INV_B - 1) / INV_B) * INV_B; }
// Dense solve of the reduced system (small maps; fallback of the PCG): A (upper block triangle, row-major, pitch lda = dense_pitch(n),
// followed by one INV_B x INV_B block of scratch) is completed, inverted in place by the block Gauss-Jordan above and applied
// to b.  No library call: rocSOLVER's potrf / potrs returned wrong solutions (relative errors up to 1e-2, tools/dbg_potrf.py)
// whenever a second process factored on the same GPU at the same time, and differed in the last bits from run to run next to
// this library's own side stream; they were exact and repeatable only when they ran alone.
void dense_launch_solve(hipStream_t s, double* A, int n, int lda, const double* b, double* x, int* bad)
{
    pcg_launch_coarse_complete(s, A, n, lda);                       // (ba_pcg_precond.hip: lower from upper, identity in the padding)
    dense_launch_invert(s, A, lda, A + (size_t)lda * lda, bad);
    pcg_launch_coarse_mirror(s, A, lda);
    hipLaunchKernelGGL(k_dense_matvec, dim3(nblk(n, 4)), dim3(256), 0, s, A, n, lda, b, x);
}
