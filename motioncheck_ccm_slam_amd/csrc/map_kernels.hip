// map_kernels.hip -- the three launches of ccm_create_new_map_points (LocalMapping::CreateNewMapPoints, src/Mapping.cpp:284-469).
//
// k_cnmp_match: SearchForTriangulation (ORBmatcher.cpp:739-805, no orientation filter) for every neighbour at once, one wave per
// (neighbour k, feature i1 without a map point).  The host has laid the neighbours' candidate features out by node, so the wave's
// lanes stride the node range of i1: Hamming distance, the epipole test and CheckDistEpipolarLine per lane, then one key per lane,
// (distance << 20) | (2^20 - 1 - position in the range), whose wave-wide minimum is "smallest distance, the last in node order among
// equals" -- what the sequential `dist > bestDist` test keeps, since the tests of a candidate do not depend on the running best.
//
// k_cnmp_triangulate: one thread per (k, i1); a thread with a match runs :363-448 (map_math.h), the 4x4 and its Jacobi in registers.
//
// k_cnmp_resolve: block b < n_kf decides neighbour b's rows, block n_kf only writes first[n_kf].  A feature belongs to the first
// neighbour whose pair passed every gate; block b finds that neighbour for every feature by reading the gate bytes of neighbours
// 0 .. b (n1 (b + 1) bytes), counts the winners of earlier neighbours (= first[b]), and lists its own winners in ascending i1 with a
// ballot scan per 256 features.  Blocks share nothing they write, so there is no ordering between them.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "map_types.h"

__global__ __launch_bounds__(MAP_TPB) void k_cnmp_match(MapDev D)
{
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (MAP_TPB / 64) + (threadIdx.x >> 6);
    if (w >= (long long)D.n_kf * D.n_free) return;
    const int k = (int)(w / D.n_free), i1 = D.free1[w % D.n_free];
    const MapKf& K = D.kf[k];
    const int32_t* rg = D.range + 2 * ((size_t)k * D.n_nodes + D.cnode1[i1]);
    const int start = rg[0], len = rg[1];
    const uint4* d1 = reinterpret_cast<const uint4*>(D.desc1) + 2 * (size_t)i1;
    const uint4 a0 = d1[0], a1 = d1[1];
    const MapFeat f1 = D.f1[i1];
    float l[3];
    map_epipolar_line(K.F12, f1.x, f1.y, l);
    const unsigned none = 0xFFFFFFFFu, pos_mask = (1u << MAP_POS_BITS) - 1;
    unsigned best = none;
    for (int j = lane; j < len; j += 64) {
        const size_t p = (size_t)start + j;
        const uint4* d2 = reinterpret_cast<const uint4*>(D.desc2) + 2 * p;
        const uint4 b0 = d2[0], b1 = d2[1];
        const int dist = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w)
                       + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
        if (dist <= MAP_TH_LOW && map_candidate_ok(l, K.ex, K.ey, D.f2[p])) best = min(best, ((unsigned)dist << MAP_POS_BITS) | (pos_mask - (unsigned)j));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o));
    if (lane == 0) D.mpos[(size_t)k * D.n1 + i1] = best == none ? -1 : start + (int)(pos_mask - (best & pos_mask));
}

__global__ __launch_bounds__(MAP_TPB) void k_cnmp_triangulate(MapDev D)
{
    const size_t t = (size_t)blockIdx.x * MAP_TPB + threadIdx.x;
    if (t >= (size_t)D.n_kf * D.n1) return;
    const int k = (int)(t / D.n1), i1 = (int)(t % D.n1);
    const int c = D.cnode1[i1];
    int st = MAP_NO_MATCH;
    float X[3] = { 0.0f, 0.0f, 0.0f };
    if (D.kf[k].skipped) st = MAP_SKIPPED_KF;
    else if (c == -2) st = MAP_HAS_MP;
    else if (c >= 0) {
        const int p = D.mpos[t];
        if (p >= 0) {
            float cosp;
            st = map_pair(D.cam[0], D.cam[1 + k], D.f1[i1], D.f2[p], D.ratioFactor, X, &cosp);
        }
    }
    D.gate[t] = (uint8_t)st;
    D.X[3 * t] = X[0]; D.X[3 * t + 1] = X[1]; D.X[3 * t + 2] = X[2];
}

// One text for k_cnmp_resolve and k_cnmp_resolve_frames: DEV is MapDev or MapFramesDev, IDX2 the matched feature of row t.  A macro and
// not a template: every template form tried (by reference, by value, a functor or an overload for IDX2) changed the device code of
// k_cnmp_resolve (tools/kernel_diff.py), and the existing kernels stay bit for bit what they were.  First it finds, for every feature,
// the first neighbour among 0 .. last whose pair passed every gate; first[b] = the winners of the neighbours before b; then
// neighbour b's winners are listed in ascending i1 (s_n is re-used: its readers of the last round are done at the first barrier).
#define CNMP_RESOLVE_KERNEL(NAME, DEV, IDX2) \
__global__ __launch_bounds__(MAP_TPB) void NAME(DEV D)                                                                           \
{                                                                                                                                \
    constexpr int W = MAP_TPB / 64;                                                                                              \
    __shared__ int s_n[W];                                                                                                       \
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;                                               \
    const int n1 = D.n1, last = min(b, D.n_kf - 1);                                                                              \
                                                                                                                                 \
    /* the first neighbour among 0 .. last whose pair with i1 passed every gate, or -1 */ \
    auto winner = [&](int i1) {                                                                                                  \
        for (int k = 0; k <= last; k++) if (D.gate[(size_t)k * n1 + i1] == MAP_OK) return k;                                     \
        return -1;                                                                                                               \
    };                                                                                                                           \
                                                                                                                                 \
    /* ---- first[b] = the winners of the neighbours before b; the final status of neighbour b's rows */ \
    int cnt = 0;                                                                                                                 \
    for (int i1 = tid; i1 < n1; i1 += MAP_TPB) {                                                                                 \
        const int w = winner(i1);                                                                                                \
        const bool earlier = w >= 0 && w < b;                                                                                    \
        cnt += earlier;                                                                                                          \
        if (b < D.n_kf) {                                                                                                        \
            const uint8_t g = D.gate[(size_t)b * n1 + i1];                                                                       \
            D.status[(size_t)b * n1 + i1] = (g == MAP_OK && earlier) ? (uint8_t)MAP_SUPERSEDED : g;                              \
        }                                                                                                                        \
    }                                                                                                                            \
_Pragma("unroll")                                                                                                                \
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);                                                                 \
    if (lane == 0) s_n[wave] = cnt;                                                                                              \
    __syncthreads();                                                                                                             \
    int running = 0;                                                                                                             \
_Pragma("unroll")                                                                                                                \
    for (int v = 0; v < W; v++) running += s_n[v];                                                                               \
    if (tid == 0) D.first[b] = running;                                                                                          \
    if (b >= D.n_kf) return;                                                                                                     \
                                                                                                                                 \
    /* ---- neighbour b's winners in ascending i1 */ \
    for (int base = 0; base < n1; base += MAP_TPB) {                                                                             \
        const int i1 = base + tid;                                                                                               \
        const bool mine = i1 < n1 && winner(i1) == b;                                                                            \
        const unsigned long long m = __ballot(mine);                                                                             \
        __syncthreads();  /* the readers of s_n of the last round are done */ \
        if (lane == 0) s_n[wave] = __popcll(m);                                                                                  \
        __syncthreads();                                                                                                         \
        int before = 0, total = 0;                                                                                               \
_Pragma("unroll")                                                                                                                \
        for (int v = 0; v < W; v++) { before += v < wave ? s_n[v] : 0; total += s_n[v]; }                                        \
        if (mine) {                                                                                                              \
            const int row = running + before + __popcll(m & ((1ull << lane) - 1));                                               \
            const size_t t = (size_t)b * n1 + i1;                                                                                \
            D.out_kf[row] = b; D.out_idx1[row] = i1; D.out_idx2[row] = (IDX2);                                                   \
            D.out_x3d[3 * row] = D.X[3 * t]; D.out_x3d[3 * row + 1] = D.X[3 * t + 1]; D.out_x3d[3 * row + 2] = D.X[3 * t + 2];   \
        }                                                                                                                        \
        running += total;                                                                                                        \
    }                                                                                                                            \
}                                                                                                                               

CNMP_RESOLVE_KERNEL(k_cnmp_resolve, MapDev, D.idx2[D.mpos[t]])

void map_match_launch(hipStream_t s, const MapDev& D)
{
    const long long waves = (long long)D.n_kf * D.n_free;
    if (waves > 0) hipLaunchKernelGGL(k_cnmp_match, dim3((unsigned)((waves + MAP_TPB / 64 - 1) / (MAP_TPB / 64))), dim3(MAP_TPB), 0, s, D);
}
void map_triangulate_launch(hipStream_t s, const MapDev& D)
{
    const size_t n = (size_t)D.n_kf * D.n1;
    hipLaunchKernelGGL(k_cnmp_triangulate, dim3((unsigned)((n + MAP_TPB - 1) / MAP_TPB)), dim3(MAP_TPB), 0, s, D);
}
void map_resolve_launch(hipStream_t s, const MapDev& D)
{
    hipLaunchKernelGGL(k_cnmp_resolve, dim3(D.n_kf + 1), dim3(MAP_TPB), 0, s, D);
}

// ---------------------------------------------------------------- the same three stages on frame handles
// (ccm_create_new_map_points_frames).  Nothing is flattened per call: a keyframe is a MapKfView of device pointers the handle owns.
//
// k_cnmp_match_frames: one wave per (neighbour k, feature i1 of the current keyframe).  The wave leaves at once when i1 holds a map
// point or has no node; otherwise it finds the node of i1 in neighbour k's directory by a wave-uniform binary search and its lanes
// stride that node's range in the node-ordered copies (contiguous 16-byte loads).  A candidate that holds a map point is skipped by
// one load through the order array.  Skipping inside the range keeps the subsequence order, so the key of k_cnmp_match -- smallest
// distance, the last in node order among equals -- picks the same feature.  The kernel stores that feature's index in neighbour k.
__device__ inline MapFeat map_view_feat(const MapKfView& V, int i)
{
    const int o = V.oct[i];
    return MapFeat{ V.kx[i], V.ky[i], V.sig2[o], V.sf[o] };
}

__global__ __launch_bounds__(MAP_TPB) void k_cnmp_match_frames(MapFramesDev D)
{
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * (MAP_TPB / 64) + (threadIdx.x >> 6);
    if (w >= (long long)D.n_kf * D.n1) return;
    const int k = (int)(w / D.n1), i1 = (int)(w % D.n1);
    const MapKfView& C = D.view[0];
    const MapKfView& N = D.view[1 + k];
    int32_t* out = D.midx + w;
    const int nd = C.node[i1];
    if (C.mp_id[i1] >= 0 || nd < 0) { if (lane == 0) *out = -1; return; }
    int lo = 0, hi = N.n_nodes;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (N.nodes[mid] < nd) lo = mid + 1; else hi = mid;
    }
    if (lo >= N.n_nodes || N.nodes[lo] != nd) { if (lane == 0) *out = -1; return; }
    const int start = N.first[lo], len = N.first[lo + 1] - start;
    const MapKf& K = D.kf[k];
    const uint4* d1 = reinterpret_cast<const uint4*>(C.desc) + 2 * (size_t)i1;
    const uint4 a0 = d1[0], a1 = d1[1];
    float l[3];
    map_epipolar_line(K.F12, C.kx[i1], C.ky[i1], l);
    const unsigned none = 0xFFFFFFFFu, pos_mask = (1u << MAP_POS_BITS) - 1;
    unsigned best = none;
    for (int j = lane; j < len; j += 64) {
        const size_t p = (size_t)start + j;
        if (N.mp_id[N.order[p]] >= 0) continue;
        const uint4* d2 = reinterpret_cast<const uint4*>(N.desc_o) + 2 * p;
        const uint4 b0 = d2[0], b1 = d2[1];
        const int dist = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w)
                       + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
        if (dist <= MAP_TH_LOW && map_candidate_ok(l, K.ex, K.ey, N.feat_o[p])) best = min(best, ((unsigned)dist << MAP_POS_BITS) | (pos_mask - (unsigned)j));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o));
    if (lane == 0) *out = best == none ? -1 : N.order[start + (int)(pos_mask - (best & pos_mask))];
}

__global__ __launch_bounds__(MAP_TPB) void k_cnmp_triangulate_frames(MapFramesDev D)
{
    const size_t t = (size_t)blockIdx.x * MAP_TPB + threadIdx.x;
    if (t >= (size_t)D.n_kf * D.n1) return;
    const int k = (int)(t / D.n1), i1 = (int)(t % D.n1);
    const MapKfView& C = D.view[0];
    const MapKfView& N = D.view[1 + k];
    int st = MAP_NO_MATCH;
    float X[3] = { 0.0f, 0.0f, 0.0f };
    if (D.kf[k].skipped) st = MAP_SKIPPED_KF;
    else if (C.mp_id[i1] >= 0) st = MAP_HAS_MP;
    else {
        const int i2 = D.midx[t];
        if (i2 >= 0) {
            float cosp;
            st = map_pair(*C.cam, *N.cam, map_view_feat(C, i1), map_view_feat(N, i2), D.ratioFactor, X, &cosp);
        }
    }
    D.gate[t] = (uint8_t)st;
    D.X[3 * t] = X[0]; D.X[3 * t + 1] = X[1]; D.X[3 * t + 2] = X[2];
}

// k_cnmp_resolve with idx2 read from midx (the match already is a feature index)
CNMP_RESOLVE_KERNEL(k_cnmp_resolve_frames, MapFramesDev, D.midx[t])

void map_frames_launch(hipStream_t s, const MapFramesDev& D)
{
    const long long pairs = (long long)D.n_kf * D.n1;
    hipLaunchKernelGGL(k_cnmp_match_frames, dim3((unsigned)((pairs + MAP_TPB / 64 - 1) / (MAP_TPB / 64))), dim3(MAP_TPB), 0, s, D);
    hipLaunchKernelGGL(k_cnmp_triangulate_frames, dim3((unsigned)((pairs + MAP_TPB - 1) / MAP_TPB)), dim3(MAP_TPB), 0, s, D);
    hipLaunchKernelGGL(k_cnmp_resolve_frames, dim3(D.n_kf + 1), dim3(MAP_TPB), 0, s, D);
}
