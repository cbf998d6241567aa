// bow_kernels.hip -- vocabulary-tree kernels.
//   k_voc_transform   DBoW2::TemplatedVocabulary::transform(feature, word, weight, nid, levelsup)
//                     (cslam/thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1217-1258): L levels of a k-way Hamming argmin
//   k_distinctive     MapPoint::ComputeDistinctiveDescriptors (cslam/src/MapPoint.cpp:957-988): least median distance
//   k_bow_directory   the FeatureVector of Frame::ComputeBoW as a keyframe handle's node directory (ccm_frame_compute_bow)
#include <hip/hip_runtime.h>
#include <cstdint>
#include "bow_directory_dev.h"

__device__ __forceinline__ int bow_ham256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1)
{
    int d = __popc(a0.x ^ b0.x);
    d += __popc(a0.y ^ b0.y); d += __popc(a0.z ^ b0.z); d += __popc(a0.w ^ b0.w);
    d += __popc(a1.x ^ b1.x); d += __popc(a1.y ^ b1.y); d += __popc(a1.z ^ b1.z); d += __popc(a1.w ^ b1.w);
    return d;
}

// One thread per feature.  The children of a node are stored side by side (slot order = the reference's children
// order), so a level is one run of k 32-byte descriptors; the k loads of a level are independent.
// node_first[n] / node_count[n] index the slot arrays; slot_node[s] is the node id of a slot.
__global__ __launch_bounds__(256) void k_voc_transform(const uint8_t* __restrict__ feat, int n, const int* __restrict__ node_first,
                                                       const int* __restrict__ node_count, const uint4* __restrict__ slot_desc,
                                                       const int* __restrict__ slot_node, const int* __restrict__ node_word,
                                                       int nid_level, int max_depth, int* __restrict__ word_id,
                                                       int* __restrict__ leaf_node, int* __restrict__ node_id)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n) return;
    const uint4* fp = reinterpret_cast<const uint4*>(feat) + 2 * (long long)f;
    const uint4 a0 = fp[0], a1 = fp[1];
    int node = 0, nid = 0;
    // max_depth bounds the loop: every lane leaves it even on a malformed tree
    for (int level = 1; level <= max_depth; level++) {
        const int cnt = node_count[node];
        if (cnt == 0) break;
        const int s = node_first[node];
        int best = 0x7fffffff, bj = 0;
        for (int j = 0; j < cnt; j++) {
            const int d = bow_ham256(a0, a1, slot_desc[2 * (long long)(s + j)], slot_desc[2 * (long long)(s + j) + 1]);
            if (d < best) { best = d; bj = j; }                 // strict <: the first of equal children wins (:1241)
        }
        node = slot_node[s + bj];
        if (level == nid_level) nid = node;
    }
    word_id[f] = node_word[node];
    leaf_node[f] = node;
    node_id[f] = nid;
}

// One wave per map point; lane i owns row i of the distance matrix (rows beyond 64 in further rounds).  The median
// of a row = the value v with  #(d <= v) > k  and  #(d <= v-1) <= k,  k = (int)(0.5 * (N - 1)): found by bisection on
// v in [0, 256] with the distances recomputed each step (N is small, the descriptors stay in L1).
__global__ __launch_bounds__(256) void k_distinctive(const uint4* __restrict__ desc, const long long* __restrict__ first,
                                                     const int* __restrict__ count, int n_points, int* __restrict__ best_out)
{
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= n_points) return;
    const int N = count[p];
    if (N <= 0) { if (lane == 0) best_out[p] = -1; return; }
    const uint4* D = desc + 2 * first[p];
    const int k = (int)(0.5 * (N - 1));
    unsigned best_key = 0xFFFFFFFFu;                             // (median << 16 | row): min = least median, first row
    for (int i = lane; i < N; i += 64) {
        const uint4 a0 = D[2 * (long long)i], a1 = D[2 * (long long)i + 1];
        int lo = 0, hi = 256;                                    // smallest v with count(d <= v) > k
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            int c = 0;
            for (int j = 0; j < N; j++) {
                const int d = j == i ? 0 : bow_ham256(a0, a1, D[2 * (long long)j], D[2 * (long long)j + 1]);
                c += d <= mid ? 1 : 0;
            }
            if (c > k) hi = mid; else lo = mid + 1;
        }
        const unsigned key = ((unsigned)lo << 16) | (unsigned)min(i, 0xFFFF);
        best_key = min(best_key, key);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best_key = min(best_key, (unsigned)__shfl_xor((int)best_key, d, 64));
    if (lane == 0) best_out[p] = (int)(best_key & 0xFFFFu);
}

// The node directory of bow_directory.h built on the device from the transform's per-feature results: node[i] = nid[i], or -1 when
// the word feature i landed in is stopped (pos[leaf[i]] == 0; TemplatedVocabulary::transform :1170-1190), then the features that
// have a node ordered by (node, feature index), the distinct nodes ascending and their first positions.  One workgroup with the
// nodes staged in LDS: rank(i) = #{node_j < node_i} + #{j < i : node_j == node_i} is the position of feature i in that stable
// order (every lane reads the same LDS word at a time: a broadcast, no bank conflict); the heads of the node runs are then numbered
// by a scan over per-thread chunks.  n <= kBowDirMax; larger frames take the host build.
__global__ __launch_bounds__(1024) void k_bow_directory(BowDirArgs A)
{
    __shared__ __attribute__((aligned(16))) int key[kBowDirMax];
    __shared__ int sorted[kBowDirMax];
    __shared__ int wsum[16];
    __shared__ int n_bow_s;
    const int t = threadIdx.x, n = A.n, lane = t & 63, w = t >> 6;
    const int NONE = 0x7fffffff;                                // sorts behind every node; never equal to one
    const int n4 = (n + 3) & ~3;
    if (t == 0) n_bow_s = 0;
    for (int i = t; i < n4; i += 1024) {
        int nd = -1;
        if (i < n) {
            if (A.leaf && A.pos[A.leaf[i]]) nd = A.nid[i];
            A.node[i] = nd;
            if (A.node_copy) A.node_copy[i] = nd;
        }
        key[i] = nd >= 0 ? nd : NONE;
    }
    __syncthreads();
    int mine = 0;
    for (int i = t; i < n; i += 1024) {
        const int k = key[i];
        if (k == NONE) continue;
        int r = 0;
        for (int j = 0; j < n4; j += 4) {
            const int4 kj = *reinterpret_cast<const int4*>(&key[j]);
            r += (kj.x < k || (kj.x == k && j < i)) ? 1 : 0;
            r += (kj.y < k || (kj.y == k && j + 1 < i)) ? 1 : 0;
            r += (kj.z < k || (kj.z == k && j + 2 < i)) ? 1 : 0;
            r += (kj.w < k || (kj.w == k && j + 3 < i)) ? 1 : 0;
        }
        A.order[r] = i;
        sorted[r] = k;
        mine++;
    }
    atomicAdd(&n_bow_s, mine);
    __syncthreads();
    const int m = n_bow_s;
    const int chunk = (m + 1023) / 1024, r0 = min(t * chunk, m), r1 = min(r0 + chunk, m);
    int heads = 0;
    for (int r = r0; r < r1; r++) heads += (r == 0 || sorted[r] != sorted[r - 1]) ? 1 : 0;
    int incl = heads;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(incl, d, 64);
        if (lane >= d) incl += u;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int base = 0, total = 0;
    for (int k = 0; k < 16; k++) { if (k < w) base += wsum[k]; total += wsum[k]; }
    int idx = base + incl - heads;
    for (int r = r0; r < r1; r++)
        if (r == 0 || sorted[r] != sorted[r - 1]) { A.nodes[idx] = sorted[r]; A.first[idx] = r; idx++; }
    if (t == 0) { A.first[total] = m; A.counts[0] = m; A.counts[1] = total; }
}

int bow_launch_directory(hipStream_t s, const BowDirArgs& A)
{
    if (A.n < 0 || A.n > kBowDirMax) return 1;
    hipLaunchKernelGGL(k_bow_directory, dim3(1), dim3(1024), 0, s, A);
    return 0;
}

void bow_launch_transform(hipStream_t s, const uint8_t* feat, int n, const int* node_first, const int* node_count, const uint8_t* slot_desc,
                          const int* slot_node, const int* node_word, int nid_level, int max_depth, int* word_id, int* leaf_node, int* node_id)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_voc_transform, dim3((n + 255) / 256), dim3(256), 0, s, feat, n, node_first, node_count,
                       reinterpret_cast<const uint4*>(slot_desc), slot_node, node_word, nid_level, max_depth, word_id, leaf_node, node_id);
}

void bow_launch_distinctive(hipStream_t s, const uint8_t* desc, const long long* first, const int* count, int n_points, int* best)
{
    if (n_points <= 0) return;
    hipLaunchKernelGGL(k_distinctive, dim3((n_points + 3) / 4), dim3(256), 0, s, reinterpret_cast<const uint4*>(desc), first, count, n_points, best);
}
