// mpt_sim3_opt_kernels.hip -- ComputeSim3's solver and optimiser on keyframe handles and the map-point table (include/ccm_hot.h
// "ComputeSim3 on handles: the solver, OptimizeSim3 and the chain"), gfx950:
//   k_sim3_solver_gather   ccm_sim3_solver_create_frames: the constructor's loop (src/Sim3Solver.cpp:30-83) in front of k_sim3_ransac
//   k_sim3_opt_gather      ccm_optimize_sim3_table_frames and the chain: the vertices and edges of src/Optimizer.cpp:937-989 in
//                          front of k_sim3_opt
//   k_sim3_chain_list / k_sim3_chain_prefix / k_sim3_chain_scatter
//                          ccm_compute_sim3_table_frames: the filter of :920-957 on the matches SearchBySim3 left in device memory, as
//                          a dense list in ascending i1, and vpMatches1[i1] = NULL back at the features
// A correspondence is a pair of features; its two map points are the slots the handles hold there.  Camera-frame points are the
// "matrix product" of the header: each row summed in double in the written order, translation included, stored as float.  Every index
// is checked before it is used as an address.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/ccm_hot.h"
#include "sim3_frames_types.h"
#include "mpt_device.h"

// The two slots and octaves of correspondence (i1, i2) of pair V, or false for a feature outside its handle, an mp_id below 0 or
// outside the table, a slot that is not LIVE or an octave outside its side's levels.  BAD is not looked at.
__device__ inline bool s3g_resolve(const Sim3FramesPair& V, const MptTable& T, int i1, int i2, int n_levels1, int n_levels2, int& s1, int& s2,
                                   int& o1, int& o2)
{
    if (i1 < 0 || i1 >= V.n1 || i2 < 0 || i2 >= V.n2) return false;
    s1 = V.mp1[i1]; s2 = V.mp2[i2];
    if (s1 < 0 || s1 >= T.capacity || s2 < 0 || s2 >= T.capacity) return false;
    if (!(T.flags[s1] & CCM_MP_LIVE) || !(T.flags[s2] & CCM_MP_LIVE)) return false;
    o1 = V.oct1[i1]; o2 = V.oct2[i2];
    return o1 >= 0 && o1 < n_levels1 && o2 >= 0 && o2 < n_levels2;
}

// blockIdx.y = the solver, so that the pair's view is the same for the whole workgroup, as in k_sim3_project.  A correspondence that
// does not resolve raises status[0] (every thread that finds one stores the same 1) and leaves zeros, which k_sim3_ransac queued
// behind can read safely; the host then reports CCM_E_ARG.
__global__ __launch_bounds__(S3G_TPB) void k_sim3_solver_gather(Sim3SolverGather G, MptTable T)
{
    const int k = blockIdx.y, j = blockIdx.x * S3G_TPB + threadIdx.x;
    const S3rSolver& S = G.solvers[k];
    if (j >= S.n) return;
    const Sim3FramesPair& V = G.pairs[k];
    const size_t e = (size_t)S.first + j;
    float X1[3] = { 0.0f, 0.0f, 0.0f }, X2[3] = { 0.0f, 0.0f, 0.0f }, m1 = 0.0f, m2 = 0.0f;
    int s1 = 0, s2 = 0, o1 = 0, o2 = 0;
    if (s3g_resolve(V, T, G.feature1[e], G.feature2[e], G.n_levels1, G.n_levels2, s1, s2, o1, o2)) {
        mpt_to_camera(V.T1w, T.pos + 3 * (size_t)s1, X1);            // :62
        mpt_to_camera(V.T2w, T.pos + 3 * (size_t)s2, X2);            // :65
        m1 = G.max_err_level1[o1]; m2 = G.max_err_level2[o2];        // :67-68, the caller's rounding
    } else G.status[0] = 1;
    for (int r = 0; r < 3; r++) { G.X1[3 * e + r] = X1[r]; G.X2[3 * e + r] = X2[r]; }
    G.max_err1[e] = m1; G.max_err2[e] = m2;
}

// blockIdx.y = the problem.  The floats widen to double as Converter::toVector3d and the Eigen assignments do.
__global__ __launch_bounds__(S3G_TPB) void k_sim3_opt_gather(Sim3OptGather G, MptTable T)
{
    const int k = blockIdx.y, j = blockIdx.x * S3G_TPB + threadIdx.x;
    const int e0 = G.first[k], e1 = G.first[k + 1];
    if (j >= e1 - e0) return;
    const Sim3FramesPair& V = G.pairs[k];
    const size_t e = (size_t)e0 + j;
    float X1[3] = { 0.0f, 0.0f, 0.0f }, X2[3] = { 0.0f, 0.0f, 0.0f }, ob1[2] = { 0.0f, 0.0f }, ob2[2] = { 0.0f, 0.0f }, w1 = 0.0f, w2 = 0.0f;
    const int i1 = G.feature1[e], i2 = G.feature2[e];
    int s1 = 0, s2 = 0, o1 = 0, o2 = 0;
    if (s3g_resolve(V, T, i1, i2, G.n_levels1, G.n_levels2, s1, s2, o1, o2)) {
        mpt_to_camera(V.T1w, T.pos + 3 * (size_t)s1, X1);            // :939
        mpt_to_camera(V.T2w, T.pos + 3 * (size_t)s2, X2);            // :947
        ob1[0] = V.kx1[i1]; ob1[1] = V.ky1[i1]; ob2[0] = V.kx2[i2]; ob2[1] = V.ky2[i2];
        w1 = G.inv_level_sigma2_1[o1]; w2 = G.inv_level_sigma2_2[o2];
    } else G.status[0] = 1;
    for (int r = 0; r < 3; r++) { G.P1[3 * e + r] = (double)X1[r]; G.P2[3 * e + r] = (double)X2[r]; }
    for (int r = 0; r < 2; r++) { G.obs1[2 * e + r] = (double)ob1[r]; G.obs2[2 * e + r] = (double)ob2[r]; }
    G.info1[e] = (double)w1; G.info2[e] = (double)w2;
}

// ---------------------------------------------------------------------------------------------------------------- the chain's list
// The feature of kf2 that feature i1 of pair P corresponds to, or -1.  A match is the solver's inlier (matched12 >= 0, at
// matched_idx2) or SearchBySim3's (match12); it becomes a correspondence when both features hold a LIVE slot that is not BAD and
// 0 <= i2 < N2 (:933-935).  Any other match is left alone.
__device__ inline int s3l_correspondence(const Sim3ChainArgs& A, const Sim3Pair& P, const Sim3FramesPair& V, const MptTable& T, int i1)
{
    const int f = P.first1 + i1;
    const int i2 = A.matched12[f] >= 0 ? A.matched_idx2[f] : A.match12[f];
    if (i2 < 0 || i2 >= P.n2) return -1;
    const int s1 = V.mp1[i1], s2 = V.mp2[i2];
    if (s1 < 0 || s1 >= T.capacity || s2 < 0 || s2 >= T.capacity) return -1;
    const uint8_t f1 = T.flags[s1], f2 = T.flags[s2];
    return (f1 & CCM_MP_LIVE) && !(f1 & CCM_MP_BAD) && (f2 & CCM_MP_LIVE) && !(f2 & CCM_MP_BAD) ? i2 : -1;
}

// One workgroup per pair walks the features of side 1 in order, S3L_TPB at a time: a wave's correspondences take consecutive rows by
// ballot, the waves in order by their counts in LDS.  place == 0 counts into cnt[pair]; place == 1 writes the rows from first[pair] on.
__global__ __launch_bounds__(S3L_TPB) void k_sim3_chain_list(Sim3ChainArgs A, MptTable T, int place)
{
    __shared__ int s_wave[S3L_TPB / 64];
    const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Sim3Pair P = A.pairs[p];
    const Sim3FramesPair& V = A.views[p];
    int row = place ? A.first[p] : 0;
    for (int i0 = 0; i0 < P.n1; i0 += S3L_TPB) {
        const int i1 = i0 + threadIdx.x;
        const int i2 = i1 < P.n1 ? s3l_correspondence(A, P, V, T, i1) : -1;
        const unsigned long long ball = __ballot(i2 >= 0);
        if (lane == 0) s_wave[wave] = __popcll(ball);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < S3L_TPB / 64; w++) { if (w < wave) before += s_wave[w]; all += s_wave[w]; }
        if (place && i2 >= 0) {
            const int r = row + before + __popcll(ball & ((1ull << lane) - 1ull));
            if (r >= 0 && r < A.n_rows) { A.feature1[r] = i1; A.feature2[r] = i2; }      // cannot fail: at most one row per feature
        }
        row += all;
        __syncthreads();
    }
    if (!place && threadIdx.x == 0) A.cnt[p] = row;
}

// first[] = the exclusive prefix of cnt[] over at most 32767 pairs, one workgroup: a run of pairs per thread
__global__ __launch_bounds__(256) void k_sim3_chain_prefix(int n, const int* cnt, int* first)
{
    __shared__ int s[256];
    const int chunk = (n + 255) / 256, lo = min(n, (int)threadIdx.x * chunk), hi = min(n, lo + chunk);
    int sum = 0;
    for (int j = lo; j < hi; j++) sum += cnt[j];
    s[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; t++) { const int v = s[t]; s[t] = run; run += v; }
        first[n] = run;
    }
    __syncthreads();
    int run = s[threadIdx.x];
    for (int j = lo; j < hi; j++) { first[j] = run; run += cnt[j]; }
}

// blockIdx.y = the pair; one thread per row
__global__ __launch_bounds__(S3G_TPB) void k_sim3_chain_scatter(Sim3ChainArgs A, const uint8_t* inlier, uint8_t* pruned)
{
    const int p = blockIdx.y, j = blockIdx.x * S3G_TPB + threadIdx.x;
    const int e0 = A.first[p], e1 = A.first[p + 1];
    if (j >= e1 - e0) return;
    const Sim3Pair P = A.pairs[p];
    const int i1 = A.feature1[e0 + j];
    if (!inlier[e0 + j] && i1 >= 0 && i1 < P.n1) pruned[P.first1 + i1] = 1;             // :1017, :1051
}

// ---------------------------------------------------------------------------------------------------------------- launchers
void sim3_solver_gather_launch(hipStream_t s, const Sim3SolverGather& G, const MptTable& T, int n_solvers, int max_n)
{
    if (n_solvers > 0 && max_n > 0)
        hipLaunchKernelGGL(k_sim3_solver_gather, dim3((max_n + S3G_TPB - 1) / S3G_TPB, n_solvers), dim3(S3G_TPB), 0, s, G, T);
}
void sim3_opt_gather_launch(hipStream_t s, const Sim3OptGather& G, const MptTable& T, int n_problems, int max_n)
{
    if (n_problems > 0 && max_n > 0)
        hipLaunchKernelGGL(k_sim3_opt_gather, dim3((max_n + S3G_TPB - 1) / S3G_TPB, n_problems), dim3(S3G_TPB), 0, s, G, T);
}
void sim3_chain_list_launch(hipStream_t s, const Sim3ChainArgs& A, const MptTable& T)
{
    if (A.n_pairs <= 0) return;
    hipLaunchKernelGGL(k_sim3_chain_list, dim3(A.n_pairs), dim3(S3L_TPB), 0, s, A, T, 0);
    hipLaunchKernelGGL(k_sim3_chain_prefix, dim3(1), dim3(256), 0, s, A.n_pairs, A.cnt, A.first);
    hipLaunchKernelGGL(k_sim3_chain_list, dim3(A.n_pairs), dim3(S3L_TPB), 0, s, A, T, 1);
}
void sim3_chain_scatter_launch(hipStream_t s, const Sim3ChainArgs& A, int max_n1, const uint8_t* inlier, uint8_t* pruned)
{
    if (A.n_pairs > 0 && max_n1 > 0)
        hipLaunchKernelGGL(k_sim3_chain_scatter, dim3((max_n1 + S3G_TPB - 1) / S3G_TPB, A.n_pairs), dim3(S3G_TPB), 0, s, A, inlier, pruned);
}
