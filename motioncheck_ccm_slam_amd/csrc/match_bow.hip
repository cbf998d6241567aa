// match_bow.hip -- SearchByBoW on the device: the greedy acceptance per vocabulary node and the rotation filter, on host-built
// group lists (ccm_match_bow) and on frame handles (the other matcher files: match_types.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include "match_types.h"
#include "match_device.h"

// ORBmatcher::SearchByBoW on the device (cslam/src/ORBmatcher.cpp:178-306 and :565-698).  A side-2 feature belongs to
// exactly one vocabulary node, so the reference's sequential "already matched" bookkeeping only couples features of the
// SAME node: one wave per node group walks its side-1 features in order (the reference's order), lanes scan the node's
// side-2 features, and the wave keeps (best, second) exactly as the if / else-if of :233-245 does -- best = first
// minimal distance in scan order, second = second smallest including duplicates.  Accepted matches mark their side-2
// feature taken, vote in the rotation histogram (integer counts), and k_bow_filter applies ComputeThreeMaxima
// (:1607-1648) and drops the matches of the other bins (:271-289).
// one wave, one node group: shared by k_bow_greedy and its batched form
__device__ __forceinline__ void bow_greedy_group(const BowDev& B, int grp, int lane)
{
    if (grp >= B.n_groups) return;
    const int a0 = B.ga[grp], a1 = B.gae[grp], b0 = B.gb[grp], b1 = B.gbe[grp];
    for (int a = a0; a < a1; a++) {
        const int i1 = B.ord1[a];
        if (!B.valid1[i1]) continue;                                 // wave-uniform
        const uint4* D1 = reinterpret_cast<const uint4*>(B.d1); const uint4* D2 = reinterpret_cast<const uint4*>(B.d2);
        const uint4 q0 = D1[2 * (long long)i1], q1 = D1[2 * (long long)i1 + 1];
        int bd1 = 256, bd2 = 256, bi = -1;
        for (int base = b0; base < b1; base += 64) {
            const int j = base + lane;
            int d = 1 << 20, i2 = -1;                                // lanes without a candidate never win
            if (j < b1) {
                i2 = B.ord2[j];
                if (!B.taken[i2] && (!B.valid2 || B.valid2[i2])) d = ham256(q0, q1, D2[2 * (long long)i2], D2[2 * (long long)i2 + 1]);
            }
            // chunk best = first minimal distance in lane (= scan) order; chunk second = smallest of the other lanes
            unsigned key = ((unsigned)d << 6) | (unsigned)lane;
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, s, 64));
            const int cb = (int)(key >> 6), cl = (int)(key & 63u);
            int o = lane == cl ? (1 << 20) : d;
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) o = min(o, __shfl_xor(o, s, 64));
            const int ci2 = __shfl(i2, cl, 64);
            // fold the chunk into the running pair the way the sequential if / else-if would
            if (cb < bd1) { bd2 = min(bd1, o); bd1 = cb; bi = ci2; }
            else bd2 = min(bd2, cb);
        }
        const bool pass = B.strict_th ? (bd1 < B.th) : (bd1 <= B.th);
        if (bi >= 0 && pass && (float)bd1 < B.nnratio * (float)bd2) {
            if (lane == 0) {
                B.match12[i1] = bi;
                B.taken[bi] = 1;
                if (B.check_ori) {
                    const int bin = rot_bin(B.angle1[i1] - B.angle2[bi]);
                    B.bin_of[i1] = bin;
                    atomicAdd(&B.hist[bin], 1);
                }
            }
            __threadfence_block();                                   // the taken flag is read by this wave's next feature
        }
    }
}
__global__ __launch_bounds__(256) void k_bow_greedy(BowDev B)
{
    bow_greedy_group(B, blockIdx.x * 4 + (threadIdx.x >> 6), threadIdx.x & 63);
}
// one workgroup: ComputeThreeMaxima on the 30 bin counts, then every match outside the kept bins is dropped
__device__ __forceinline__ void bow_filter_block(const BowDev& B)
{
    __shared__ int keep[3];
    __shared__ int cnt;
    if (threadIdx.x == 0) {
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        if (B.check_ori) {
            for (int i = 0; i < 30; i++) {
                const int s = B.hist[i];
                if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
                else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
                else if (s > max3) { max3 = s; ind3 = i; }
            }
            if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
            else if (max3 < 0.1f * (float)max1) ind3 = -1;
        }
        keep[0] = ind1; keep[1] = ind2; keep[2] = ind3; cnt = 0;
    }
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < B.n1; i += 256) {
        if (B.match12[i] < 0) continue;
        if (B.check_ori) {
            const int b = B.bin_of[i];
            if (b != keep[0] && b != keep[1] && b != keep[2]) { B.match12[i] = -1; continue; }
        }
        mine++;
    }
    atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) B.hist[30] = cnt;
}
__global__ __launch_bounds__(256) void k_bow_filter(BowDev B) { bow_filter_block(B); }
void match_launch_bow(hipStream_t s, const BowDev& B)
{
    if (B.n_groups > 0) hipLaunchKernelGGL(k_bow_greedy, dim3((B.n_groups + 3) / 4), dim3(256), 0, s, B);
    hipLaunchKernelGGL(k_bow_filter, dim3(1), dim3(256), 0, s, B);
}

// ------------------------------------------------------------------------------------------------
// SearchByBoW on frame handles (ccm_frame_search_by_bow, ccm_search_by_bow_frames): both sides carry their node directory (order |
// nodes | first, ccm_frame_set_bow / ccm_frame_compute_bow) in device memory, so the group list ccm_match_bow merges on the host
// is made here.  One record per pair; the batched forms take the pair from blockIdx.y.
// One thread per distinct node of side 1 looks its node up in side 2's ascending `nodes` and writes the two position ranges
// (both empty when side 2 lacks the node); the same launch clears taken, match12, match21 and the histogram and derives the masks.
template <bool BATCH>
__global__ __launch_bounds__(256) void k_bow_groups(BowFrameRec one, const BowFrameRec* __restrict__ recs)
{
    const BowFrameRec R = BATCH ? recs[blockIdx.y] : one;
    const BowDev& B = R.B;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < B.n_groups) {
        const int nd = R.nodes1[t];
        int lo = 0, hi = R.n_nodes2;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (R.nodes2[mid] < nd) lo = mid + 1; else hi = mid;
        }
        const bool hit = lo < R.n_nodes2 && R.nodes2[lo] == nd;
        const_cast<int*>(B.ga)[t] = hit ? R.first1[t] : 0; const_cast<int*>(B.gae)[t] = hit ? R.first1[t + 1] : 0;
        const_cast<int*>(B.gb)[t] = hit ? R.first2[lo] : 0; const_cast<int*>(B.gbe)[t] = hit ? R.first2[lo + 1] : 0;
    }
    if (t < B.n1) {
        B.match12[t] = -1;
        if (R.v1 && (!BATCH || blockIdx.y == 0)) R.v1[t] = R.mp1[t] >= 0 ? 1 : 0;      // one mask of side 1 serves every pair
    }
    if (t < R.n2) {
        B.taken[t] = 0;
        if (R.v2) R.v2[t] = R.mp2[t] >= 0 ? 1 : 0;
        if (R.match21) R.match21[t] = -1;
    }
    if (t < 32) B.hist[t] = 0;
}
__global__ __launch_bounds__(256) void k_bow_greedy_batch(const BowFrameRec* __restrict__ recs)
{
    const BowDev B = recs[blockIdx.y].B;
    bow_greedy_group(B, blockIdx.x * 4 + (threadIdx.x >> 6), threadIdx.x & 63);
}
__global__ __launch_bounds__(256) void k_bow_filter_batch(const BowFrameRec* __restrict__ recs)
{
    const BowDev B = recs[blockIdx.x].B;
    bow_filter_block(B);
}
// Frame overload: vpMapPointMatches[idx2] = MP(idx1) (:251) -- match12 inverted (a side-2 feature is taken at most once), and,
// when nmatches >= min_matches, the frame's mp_id replaced as a whole (Tracking.cpp:529).  One workgroup.
__global__ __launch_bounds__(1024) void k_bow_invert(BowFrameRec R, int min_matches, int* __restrict__ mp_id2)
{
    const BowDev& B = R.B;
    for (int i1 = threadIdx.x; i1 < B.n1; i1 += 1024) {
        const int m = B.match12[i1];
        if (m >= 0) R.match21[m] = i1;
    }
    __syncthreads();
    if (B.hist[30] < min_matches) return;
    for (int i2 = threadIdx.x; i2 < R.n2; i2 += 1024) {
        const int m = R.match21[i2];
        mp_id2[i2] = m >= 0 ? R.mp1[m] : -1;
    }
}
void match_launch_bow_groups(hipStream_t s, const BowFrameRec& one, const BowFrameRec* recs, int n_recs, int max_threads)
{
    const dim3 grid((std::max(max_threads, 32) + 255) / 256, recs ? n_recs : 1);
    if (recs) hipLaunchKernelGGL(k_bow_groups<true>, grid, dim3(256), 0, s, one, recs);
    else hipLaunchKernelGGL(k_bow_groups<false>, grid, dim3(256), 0, s, one, recs);
}
void match_launch_bow_batch(hipStream_t s, const BowFrameRec* recs, int n_recs, int n_groups)
{
    if (n_groups > 0) hipLaunchKernelGGL(k_bow_greedy_batch, dim3((n_groups + 3) / 4, n_recs), dim3(256), 0, s, recs);
    hipLaunchKernelGGL(k_bow_filter_batch, dim3(n_recs), dim3(256), 0, s, recs);
}
void match_launch_bow_invert(hipStream_t s, const BowFrameRec& R, int min_matches, int* mp_id2)
{
    hipLaunchKernelGGL(k_bow_invert, dim3(1), dim3(1024), 0, s, R, min_matches, mp_id2);
}
