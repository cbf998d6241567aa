// mpt_kernels.hip -- device side of the map-point table (mpt_host.cpp, include/ccm_hot.h "map-point table"):
//   k_mpt_scatter      rows of a ccm_map_update into the table's columns
//   k_mpt_gather       test tap: rows of a slot list out of the table
//   k_slp_mark         first loop of Tracking::SearchLocalPoints (src/Tracking.cpp:863-879), thread per frame feature
//   k_slp_frustum      second loop (:888-908): Frame::isInFrustum (src/Frame.cpp:139-198) and MapPoint::PredictScale
//                      (src/MapPoint.cpp:854-869), thread per entry of the order list; per-wave ballots, per-workgroup counts
//   k_slp_scan         exclusive scan of the workgroup counts, one workgroup; the in-view count
//   k_slp_compact      the entries in view, in list order, into the query arrays of the windowed matcher
//   k_mpt_refresh      MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:929-994) and MapPoint::UpdateNormalAndDepth (:779-823)
//                      for a list of points whose observations name keyframe handles; one wave per point
//   k_fuse_where / k_fuse_held / k_fuse_project / k_fuse_scatter
//                      ccm_fuse_select_table_frames: the projection and the gates of ORBmatcher::Fuse, both overloads
//                      (src/ORBmatcher.cpp:870-920, :1018-1071), for every (keyframe, point) pair; the survivors become the
//                      queries of k_window_select (match_window.hip)
//   k_tmm_project / k_tmm_clear / k_tmm_discard
//                      ccm_frame_track_motion_model: the queries of SearchByProjection(Current, Last) from the last frame's ids
//                      (src/ORBmatcher.cpp:1374-1396), the clear before each pass and "discard outliers" (src/Tracking.cpp:599-618)
// No kernel waits for another workgroup: the compaction is three launches (ballot + count, scan, scatter).
// Every index is checked against the table's capacity before it is used as an address.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/ccm_hot.h"
#include "mpt_types.h"
#include "mpt_device.h"

// ---------------------------------------------------------------------------------------------------------------- table rows
__global__ void k_mpt_scatter(MptTable T, int n, const int* slot, const float* pos, const float* normal, const float* min_dist,
                              const float* max_dist, const uint8_t* desc, const uint8_t* flags)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int s = slot[r];
    if (s < 0 || s >= T.capacity) return;        // < 0: superseded by a later row of the same slot (the host marks them)
    if (pos) for (int d = 0; d < 3; d++) T.pos[3 * (size_t)s + d] = pos[3 * (size_t)r + d];
    if (normal) for (int d = 0; d < 3; d++) T.normal[3 * (size_t)s + d] = normal[3 * (size_t)r + d];
    if (min_dist) T.min_dist[s] = min_dist[r];
    if (max_dist) T.max_dist[s] = max_dist[r];
    if (desc) {
        const uint4* a = reinterpret_cast<const uint4*>(desc + (size_t)r * 32);
        uint4* b = reinterpret_cast<uint4*>(T.desc + (size_t)s * 32);
        b[0] = a[0]; b[1] = a[1];
    }
    if (flags) T.flags[s] = flags[r];
}

__global__ void k_mpt_gather(MptTable T, int n, const int* slot, float* pos, float* normal, float* min_dist, float* max_dist, uint8_t* desc,
                             uint8_t* flags, int* seen)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int s = slot[r];
    if (s < 0 || s >= T.capacity) return;
    for (int d = 0; d < 3; d++) { pos[3 * (size_t)r + d] = T.pos[3 * (size_t)s + d]; normal[3 * (size_t)r + d] = T.normal[3 * (size_t)s + d]; }
    min_dist[r] = T.min_dist[s]; max_dist[r] = T.max_dist[s];
    const uint4* a = reinterpret_cast<const uint4*>(T.desc + (size_t)s * 32);
    uint4* b = reinterpret_cast<uint4*>(desc + (size_t)r * 32);
    b[0] = a[0]; b[1] = a[1];
    flags[r] = T.flags[s]; seen[r] = T.seen[s];
}

// ---------------------------------------------------------------------------------------------------------------- first loop
// ids / occ / match lie in the call's result block; the handle's own mp_id is replaced by ids only once the host has seen bad == 0.
__global__ void k_slp_mark(MptTable T, int n, const int* mp_id, int stamp, int* ids, uint8_t* occ, int* match, int* cnt)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int id = mp_id[i];
    uint8_t o = 0;
    if (id >= 0) {
        const uint8_t fl = id < T.capacity ? T.flags[id] : 0;
        if (!(fl & CCM_MP_LIVE)) cnt[1] = 1;                    // outside the table or not in use: the host reports CCM_E_ARG
        else if (fl & CCM_MP_BAD) id = -1;                      // :868-871
        else { T.seen[id] = stamp; o = (fl & CCM_MP_HAS_OBS) ? 1 : 0; }   // :875; several features may hold one slot: same value
    }
    ids[i] = id; occ[i] = o; match[i] = -1;
}

// ---------------------------------------------------------------------------------------------------------------- second loop
__device__ inline int slp_slot(const SlpArgs& A, int j) { return A.order ? A.order[j] : j; }

// (mpt_to_camera and mpt_pinhole, the projection of SearchLocalPoints and TrackWithMotionModel: mpt_device.h)

// Frame::isInFrustum + PredictScale for one point, in the arithmetic of float cv::Mat expressions (map_math.h: the products of
// a matrix product, dot and norm are summed in double and stored as float; everything else is float, left to right).
__device__ inline bool slp_in_frustum(const SlpArgs& A, const MptTable& T, int s, float& u, float& v, float& view_cos, int& level)
{
    const float P[3] = { T.pos[3 * (size_t)s], T.pos[3 * (size_t)s + 1], T.pos[3 * (size_t)s + 2] };
    float Pc[3];
    mpt_to_camera(A.Tcw, P, Pc);
    if (Pc[2] < 0.0f) return false;
    const float invz = 1.0f / Pc[2];
    mpt_pinhole(A.fx, A.fy, A.cx, A.cy, Pc, invz, u, v);
    if (u < A.min_x || u > A.max_x) return false;
    if (v < A.min_y || v > A.max_y) return false;
    const float max_d = T.max_dist[s];
    const float PO[3] = { P[0] - A.Ow[0], P[1] - A.Ow[1], P[2] - A.Ow[2] };
    const float dist = (float)sqrt((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1] + (double)PO[2] * (double)PO[2]);
    if (dist < 0.8f * T.min_dist[s] || dist > 1.2f * max_d) return false;
    const double dot = (double)PO[0] * (double)T.normal[3 * (size_t)s] + (double)PO[1] * (double)T.normal[3 * (size_t)s + 1] +
                       (double)PO[2] * (double)T.normal[3 * (size_t)s + 2];
    view_cos = (float)(dot / (double)dist);
    if (view_cos < A.cos_limit) return false;
    const float ratio = max_d / dist;
    const float lg = (float)log((double)ratio);
    const float q = ceilf(lg / A.log_scale);
    level = !(q >= 0.0f) ? 0 : (q >= (float)A.n_levels ? A.n_levels - 1 : (int)q);
    return true;
}

// One thread per entry of the order list, SLP_TPB / 64 waves per workgroup.  mask[j / 64] = the wave's ballot, wg_cnt[b] = entries in
// view of workgroup b; tmp_* hold the values of the entries in view at their list position.
__global__ __launch_bounds__(SLP_TPB) void k_slp_frustum(SlpArgs A, MptTable T)
{
    __shared__ int s_cnt[SLP_TPB / 64];
    const int j = blockIdx.x * SLP_TPB + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bool keep = false;
    if (j < A.n_order) {
        const int s = slp_slot(A, j);
        if (s >= 0 && s < T.capacity) {
            const uint8_t fl = T.flags[s];
            if ((fl & CCM_MP_LIVE) && !(fl & CCM_MP_BAD) && T.seen[s] != A.stamp) {     // :891-900
                float u, v, vc; int level;
                keep = slp_in_frustum(A, T, s, u, v, vc, level);
                if (keep) { A.tmp_u[j] = u; A.tmp_v[j] = v; A.tmp_vc[j] = vc; A.tmp_level[j] = level; }
            }
        }
    }
    const unsigned long long ball = __ballot(keep);
    if (lane == 0) {
        s_cnt[wv] = __popcll(ball);
        if (blockIdx.x * SLP_TPB + wv * 64 < A.n_order) A.mask[(size_t)blockIdx.x * (SLP_TPB / 64) + wv] = ball;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < SLP_TPB / 64; w++) t += s_cnt[w];
        A.wg_cnt[blockIdx.x] = t;
    }
}

// Exclusive scan of wg_cnt [n_wg] into wg_off, one workgroup of SCAN_TPB threads walking the array in chunks; cnt[0] = the total.
__global__ __launch_bounds__(SCAN_TPB) void k_slp_scan(int n_wg, const int* wg_cnt, int* wg_off, int* cnt)
{
    __shared__ int s_v[SCAN_TPB];
    __shared__ int s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int base = 0; base < n_wg; base += SCAN_TPB) {
        const int i = base + tid;
        const int mine = i < n_wg ? wg_cnt[i] : 0;
        s_v[tid] = mine;
        __syncthreads();
        for (int off = 1; off < SCAN_TPB; off <<= 1) {
            const int v = tid >= off ? s_v[tid - off] : 0;
            __syncthreads();
            s_v[tid] += v;
            __syncthreads();
        }
        if (i < n_wg) wg_off[i] = s_base + s_v[tid] - mine;
        __syncthreads();
        if (tid == 0) s_base += s_v[SCAN_TPB - 1];
        __syncthreads();
    }
    if (tid == 0) cnt[0] = s_base;
}

// Entry j in view goes to k = wg_off[b] + (entries in view of the workgroup's earlier waves) + (earlier lanes of its wave): list order
// is kept.  Query set-up exactly as window_queries_projection() (match_window_host.cpp; ORBmatcher.cpp:97-107, RadiusByViewingCos :150-156).
__global__ __launch_bounds__(SLP_TPB) void k_slp_compact(SlpArgs A, MptTable T)
{
    const int j = blockIdx.x * SLP_TPB + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (j >= A.n_order) return;
    const unsigned long long* m = A.mask + (size_t)blockIdx.x * (SLP_TPB / 64);
    const unsigned long long mine = m[wv];
    if (!((mine >> lane) & 1ull)) return;
    int k = A.wg_off[blockIdx.x] + __popcll(mine & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; w++) k += __popcll(m[w]);
    if (k < 0 || k >= A.n_order) return;         // cannot happen: at most n_order entries are in view
    const int s = slp_slot(A, j);
    const float vc = A.tmp_vc[j];
    const int level = A.tmp_level[j];
    float r = (double)vc > 0.998 ? 2.5f : 4.0f;
    if (A.th != 1.0f) r *= A.th;
    A.qx[k] = A.tmp_u[j]; A.qy[k] = A.tmp_v[j]; A.qr[k] = r * A.scale[level];
    A.minl[k] = level - 1; A.maxl[k] = level;
    A.qact[k] = 1; A.qflag[k] = (T.flags[s] & CCM_MP_HAS_OBS) ? 1 : 0;
    A.slots[k] = s;
    A.tap_level[k] = level; A.tap_vc[k] = vc;
    const uint4* a = reinterpret_cast<const uint4*>(T.desc + (size_t)s * 32);
    uint4* b = reinterpret_cast<uint4*>(A.qdesc + (size_t)k * 32);
    b[0] = a[0]; b[1] = a[1];
}

// ---------------------------------------------------------------------------------------------------------------- refresh
// One wave per listed map point, MPR_TPB / 64 points per workgroup (as k_distinctive, bow_kernels.hip).
//   Gather: lane i fetches observation i's 32 bytes from its keyframe's descriptor rows into the wave's LDS copy -- the only scattered
//   traffic, about one cache line per observation.  The copy holds MPR_LDS_ROWS rows; the rows of a longer list are read through the
//   index lists from global memory wherever they are needed, so any count is handled.
//   Median: lane i owns row i of the distance matrix (rows beyond 64 in further rounds) and bisects [0, 256] for the smallest v with
//   #(d <= v) > k, k = (int)(0.5 * (c - 1)); all lanes read the same column at a time (an LDS broadcast).  The least (median, row)
//   over the wave is the choice: among equal medians the first observation wins.
//   Normal: lanes compute the unit rays of their observations in parallel; the sum is then taken strictly in list order, every lane
//   adding the same values handed round by __shfl (a float sum depends on its order; a tree would give another result).
// The arithmetic is that of float cv::Mat expressions (include/ccm_hot.h, ccm_map_table_refresh): norms summed in double, the
// multiply and the add of scaleAdd rounded separately.  No atomics, no scratch; every slot is checked against the capacity.
__device__ inline const uint4* mpr_row(const MptRefreshArgs& A, int e)
{
    return reinterpret_cast<const uint4*>(A.view[A.obs_kf[e]].desc + 32 * (size_t)A.obs_feat[e]);
}
__device__ inline int mpr_ham256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1)
{
    int d = __popc(a0.x ^ b0.x);
    d += __popc(a0.y ^ b0.y); d += __popc(a0.z ^ b0.z); d += __popc(a0.w ^ b0.w);
    d += __popc(a1.x ^ b1.x); d += __popc(a1.y ^ b1.y); d += __popc(a1.z ^ b1.z); d += __popc(a1.w ^ b1.w);
    return d;
}
// cv::norm of a float 3-vector: the squares summed in double
__device__ inline double mpr_norm(float x, float y, float z)
{
    return sqrt(__dadd_rn(__dadd_rn(__dmul_rn((double)x, (double)x), __dmul_rn((double)y, (double)y)), __dmul_rn((double)z, (double)z)));
}

__global__ __launch_bounds__(MPR_TPB) void k_mpt_refresh(MptRefreshArgs A, MptTable T)
{
    __shared__ uint4 s_desc[MPR_TPB / 64][2 * MPR_LDS_ROWS];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, p = blockIdx.x * (MPR_TPB / 64) + wv;
    int c = 0, o0 = 0, s = -1;
    if (p < A.n) { o0 = A.obs_first[p]; c = A.obs_first[p + 1] - o0; s = A.slot[p]; }
    const bool in_table = s >= 0 && s < T.capacity;             // the host has checked it
    const bool do_desc = in_table && c > 0 && (A.what & CCM_MPR_DESCRIPTOR);
    const bool do_nd = in_table && c > 0 && (A.what & CCM_MPR_NORMAL_DEPTH);
    const int n_lds = do_desc ? min(c, MPR_LDS_ROWS) : 0;
    uint4* L = s_desc[wv];
    for (int i = lane; i < n_lds; i += 64) {
        const uint4* g = mpr_row(A, o0 + i);
        L[2 * i] = g[0]; L[2 * i + 1] = g[1];
    }
    __syncthreads();                                             // every wave comes here once, whatever its point
    if (!in_table) return;

    float P0, P1, P2;
    if (A.pos) {
        P0 = A.pos[3 * (size_t)p]; P1 = A.pos[3 * (size_t)p + 1]; P2 = A.pos[3 * (size_t)p + 2];
        if (lane == 0) { T.pos[3 * (size_t)s] = P0; T.pos[3 * (size_t)s + 1] = P1; T.pos[3 * (size_t)s + 2] = P2; }
    } else {
        P0 = T.pos[3 * (size_t)s]; P1 = T.pos[3 * (size_t)s + 1]; P2 = T.pos[3 * (size_t)s + 2];
    }
    if (A.flags && lane == 0) T.flags[s] = A.flags[p];

    int best = -1;
    if (do_desc) {
        const int k = (int)(0.5 * (c - 1));
        int med = 0x7fffffff, row = 0x7fffffff;
        for (int i = lane; i < c; i += 64) {
            uint4 a0, a1;
            if (i < n_lds) { a0 = L[2 * i]; a1 = L[2 * i + 1]; }
            else { const uint4* g = mpr_row(A, o0 + i); a0 = g[0]; a1 = g[1]; }
            int lo = 0, hi = 256;                                // smallest v with count(d <= v) > k
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                int cnt = 0;
                for (int j = 0; j < n_lds; j++) cnt += mpr_ham256(a0, a1, L[2 * j], L[2 * j + 1]) <= mid ? 1 : 0;
                for (int j = n_lds; j < c; j++) {
                    const uint4* g = mpr_row(A, o0 + j);
                    cnt += mpr_ham256(a0, a1, g[0], g[1]) <= mid ? 1 : 0;
                }
                if (cnt > k) hi = mid; else lo = mid + 1;
            }
            if (lo < med) { med = lo; row = i; }                 // rows ascend per lane: the first of equal medians stays
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int om = __shfl_xor(med, d, 64), orow = __shfl_xor(row, d, 64);
            if (om < med || (om == med && orow < row)) { med = om; row = orow; }
        }
        best = row;
        if (lane < 2) {
            const uint4 v = best < n_lds ? L[2 * best + lane] : mpr_row(A, o0 + best)[lane];
            reinterpret_cast<uint4*>(T.desc + (size_t)s * 32)[lane] = v;
        }
    }

    float n0, n1, n2, mn, mx;
    if (do_nd) {
        n0 = 0.0f; n1 = 0.0f; n2 = 0.0f;
        for (int base = 0; base < c; base += 64) {
            const int i = base + lane;
            float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
            if (i < c) {
                const float* Ow = A.view[A.obs_kf[o0 + i]].Ow;
                const float d0 = P0 - Ow[0], d1 = P1 - Ow[1], d2 = P2 - Ow[2];
                const float a = (float)(1.0 / mpr_norm(d0, d1, d2));
                v0 = __fmul_rn(d0, a); v1 = __fmul_rn(d1, a); v2 = __fmul_rn(d2, a);
            }
            const int m = min(64, c - base);
            for (int l = 0; l < m; l++) {                        // cv::scaleAdd, observation by observation
                n0 = __fadd_rn(__shfl(v0, l, 64), n0); n1 = __fadd_rn(__shfl(v1, l, 64), n1); n2 = __fadd_rn(__shfl(v2, l, 64), n2);
            }
        }
        const float inv = (float)(1.0 / (double)c);              // Mat / n multiplies by the reciprocal
        n0 = __fmul_rn(n0, inv); n1 = __fmul_rn(n1, inv); n2 = __fmul_rn(n2, inv);
        const MptKfView& R = A.view[A.ref_kf[p]];
        const float dist = (float)mpr_norm(P0 - R.Ow[0], P1 - R.Ow[1], P2 - R.Ow[2]);
        const int level = min(max(R.oct[A.ref_feat[p]], 0), 255);   // within the handle's n_levels; sf holds 256 entries
        mx = __fmul_rn(dist, R.sf[level]);
        mn = __fdiv_rn(mx, R.sf[R.n_levels - 1]);
        if (lane == 0) {
            T.normal[3 * (size_t)s] = n0; T.normal[3 * (size_t)s + 1] = n1; T.normal[3 * (size_t)s + 2] = n2;
            T.min_dist[s] = mn; T.max_dist[s] = mx;
        }
    } else {                                                     // the result block reports the row as it stands
        n0 = T.normal[3 * (size_t)s]; n1 = T.normal[3 * (size_t)s + 1]; n2 = T.normal[3 * (size_t)s + 2];
        mn = T.min_dist[s]; mx = T.max_dist[s];
    }
    if (lane == 0) {
        A.best[p] = best;
        A.normal[3 * (size_t)p] = n0; A.normal[3 * (size_t)p + 1] = n1; A.normal[3 * (size_t)p + 2] = n2;
        A.min_dist[p] = mn; A.max_dist[p] = mx;
    }
}

// ---------------------------------------------------------------------------------------------------------------- fuse
// Membership ("keyframe k already holds point j", IsInKeyFrame :877 / spAlreadyFound :1023) without a search: where[slot] = the
// call's stamp and the slot's position in the list, then every feature of every keyframe looks its mp_id up.  An entry of an earlier
// call carries an older stamp and reads as "not listed"; nothing has to be cleared.
__global__ void k_fuse_where(FuseArgs A, int capacity)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= A.n_points) return;
    const int s = A.slot[j];
    if (s >= 0 && s < capacity) A.where[s] = ((unsigned long long)A.stamp << 32) | (unsigned)j;
}
__global__ void k_fuse_held(FuseArgs A, int capacity)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    const FuseView& V = A.views[k];
    if (i >= V.n) return;
    const int id = V.mp_id[i];
    if (id < 0 || id >= capacity) return;        // an id outside the table names none of the listed points
    const unsigned long long w = A.where[id];
    const unsigned pos = (unsigned)w;
    if ((unsigned)(w >> 32) == A.stamp && pos < (unsigned)A.n_points) A.held[(size_t)k * A.n_points + pos] = 1;   // several features: same value
}

// (fuse_predict_level, MapPoint::PredictScale: mpt_device.h)

// One thread per (keyframe, point) pair; blockIdx.y = the keyframe, so the view is the same for the whole workgroup and is read
// through scalar loads.  Arithmetic of a float cv::Mat as in slp_in_frustum (products of a matrix product, dot and norm summed in
// double), but Fuse's own association of the projection: x = PcX * invz first, then fx * x + cx (:890-895, :1040-1045).
// The survivors of a wave take consecutive places of the query list behind ONE atomic add; which wave comes first is not fixed, and
// does not matter: k_window_select decides per query and k_fuse_scatter writes by pair index.
__global__ __launch_bounds__(FUSE_TPB) void k_fuse_project(FuseArgs A, MptTable T)
{
    const int j = blockIdx.x * FUSE_TPB + threadIdx.x, k = blockIdx.y, lane = threadIdx.x & 63;
    const FuseView& V = A.views[k];
    const size_t n_pairs = (size_t)A.n_kf * A.n_points, pair = (size_t)k * A.n_points + (j < A.n_points ? j : 0);
    bool keep = false;
    int gate = CCM_FG_SKIPPED, level = 0, s = -1;
    float u = 0.0f, v = 0.0f;
    if (j < A.n_points) {
        s = A.slot[j];
        uint8_t fl = 0;
        if (s >= 0 && s < T.capacity && !(A.skip && A.skip[j])) fl = T.flags[s];
        if ((fl & CCM_MP_LIVE) && !(fl & CCM_MP_BAD)) {
            gate = CCM_FG_IN_KEYFRAME;
            if (!A.held[pair]) {
                const float P[3] = { T.pos[3 * (size_t)s], T.pos[3 * (size_t)s + 1], T.pos[3 * (size_t)s + 2] };
                float Pc[3];
                for (int r = 0; r < 3; r++)
                    Pc[r] = (float)((double)V.Tcw[4 * r] * (double)P[0] + (double)V.Tcw[4 * r + 1] * (double)P[1] +
                                    (double)V.Tcw[4 * r + 2] * (double)P[2] + (double)V.Tcw[4 * r + 3]);
                gate = CCM_FG_BEHIND;
                if (!(Pc[2] < 0.0f)) {
                    const float invz = __fdiv_rn(1.0f, Pc[2]);
                    const float x = __fmul_rn(Pc[0], invz), y = __fmul_rn(Pc[1], invz);
                    u = __fadd_rn(__fmul_rn(V.fx, x), V.cx);
                    v = __fadd_rn(__fmul_rn(V.fy, y), V.cy);
                    gate = CCM_FG_OUTSIDE;
                    if (u >= V.min_x && u < V.max_x && v >= V.min_y && v < V.max_y) {      // KeyFrame::IsInImage; a NaN is outside
                        const float max_d = T.max_dist[s];
                        const float PO[3] = { P[0] - V.Ow[0], P[1] - V.Ow[1], P[2] - V.Ow[2] };
                        const float dist = (float)sqrt((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1] + (double)PO[2] * (double)PO[2]);
                        gate = CCM_FG_DISTANCE;
                        if (!(dist < 0.8f * T.min_dist[s] || dist > 1.2f * max_d)) {
                            const double dot = (double)PO[0] * (double)T.normal[3 * (size_t)s] + (double)PO[1] * (double)T.normal[3 * (size_t)s + 1] +
                                               (double)PO[2] * (double)T.normal[3 * (size_t)s + 2];
                            gate = CCM_FG_ANGLE;
                            if (!(dot < 0.5 * (double)dist)) {
                                level = fuse_predict_level(max_d, dist, A.log_scale, A.n_levels);
                                gate = V.n > 0 ? CCM_FG_SEARCHED : CCM_FG_EMPTY_KF;
                                keep = V.n > 0;
                            }
                        }
                    }
                }
            }
        }
        A.best_idx[pair] = -1;
        if (A.best_dist) A.best_dist[pair] = 256;
        if (A.gate) A.gate[pair] = (uint8_t)gate;
        if (A.u) { A.u[pair] = u; A.v[pair] = v; A.level[pair] = level; }
    }
    const unsigned long long ball = __ballot(keep);
    if (!ball) return;
    const int leader = __ffsll((long long)ball) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(A.cnt, __popcll(ball));
    base = __shfl(base, leader, 64);
    if (!keep) return;
    const size_t q = (size_t)base + __popcll(ball & ((1ull << lane) - 1ull));
    if (q >= n_pairs) return;                    // cannot happen: at most one query per pair
    A.qx[q] = u; A.qy[q] = v; A.qr[q] = A.th * A.scale[level];      // :920 / :1071
    A.minl[q] = level - 1; A.maxl[q] = level;                       // :937-938 / :1089
    A.qkf[q] = k; A.qpair[q] = (int)pair;
    const uint4* a = reinterpret_cast<const uint4*>(T.desc + (size_t)s * 32);
    uint4* b = reinterpret_cast<uint4*>(A.qdesc + q * 32);
    b[0] = a[0]; b[1] = a[1];
}

__global__ void k_fuse_scatter(int nq, int n_pairs, const int* qpair, const int* sel_i, const int* sel_d, int* best_idx, int* best_dist)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const int pair = qpair[q];
    if (pair < 0 || pair >= n_pairs) return;
    best_idx[pair] = sel_i[q];
    if (best_dist) best_dist[pair] = sel_d[q];
}

// ---------------------------------------------------------------------------------------------------------------- motion model
// ccm_frame_track_motion_model.  k_tmm_project: the first half of the loop of ORBmatcher::SearchByProjection(Current, Last)
// (src/ORBmatcher.cpp:1374-1396), one thread per feature of the last frame.  A feature without a point, or one LastFrame.mvbOutlier
// names, is no query; isBad() is not asked there, so a BAD slot is projected.  An id outside the table or of a slot that is not LIVE
// raises head[0] (every thread that finds one stores the same 1) and is never used as an address.  Stated deviation: a u or v that is
// not finite (PcZ == 0) is rejected; the reference would hand it to GetFeaturesInArea.  A feature that is no query gets u = v = 0.
__global__ __launch_bounds__(TMM_TPB) void k_tmm_project(TmmArgs A, MptTable T)
{
    const int i = blockIdx.x * TMM_TPB + threadIdx.x;
    if (i >= A.n_last) return;
    const int id = A.last_id[i];
    float u = 0.0f, v = 0.0f;
    bool valid = false;
    uint8_t fl = 0;
    if (id >= 0 && !(A.last_outlier && A.last_outlier[i])) {
        fl = id < T.capacity ? T.flags[id] : 0;
        if (!(fl & CCM_MP_LIVE)) A.head[0] = 1;
        else {
            const float P[3] = { T.pos[3 * (size_t)id], T.pos[3 * (size_t)id + 1], T.pos[3 * (size_t)id + 2] };
            float Pc[3];
            mpt_to_camera(A.Tcw, P, Pc);
            const float invz = 1.0f / Pc[2];
            if (!(invz < 0.0f)) {                                              // :1386
                mpt_pinhole(A.fx, A.fy, A.cx, A.cy, Pc, invz, u, v);
                valid = fabsf(u) <= 3.402823466e+38f && fabsf(v) <= 3.402823466e+38f &&      // a NaN compares false
                        !(u < A.min_x || u > A.max_x) && !(v < A.min_y || v > A.max_y);      // :1392-1395, both ends inside
                if (!valid) { u = 0.0f; v = 0.0f; }
            }
        }
    }
    A.qx[i] = u; A.qy[i] = v; A.act[i] = valid ? 1 : 0; A.qflag[i] = (valid && (fl & CCM_MP_HAS_OBS)) ? 1 : 0;
    if (valid) {
        const uint4* a = reinterpret_cast<const uint4*>(T.desc + (size_t)id * 32);
        uint4* b = reinterpret_cast<uint4*>(A.qdesc + (size_t)i * 32);
        b[0] = a[0]; b[1] = a[1];
    }
}

// Before every search pass (src/Tracking.cpp:579, :589): the current frame's ids to -1, the matcher's result to -1, its occupancy flags
// to 0.  With head[0] raised by k_tmm_project the ids stay as they are and every query is switched off instead, so that the pass
// queued behind finds nothing and writes nothing; the host then reports CCM_E_ARG.
__global__ void k_tmm_clear(int n_cur, int n_last, const int* head, int* mp_id, int* out, uint8_t* flag, uint8_t* act)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool bad = head[0] != 0;
    if (i < n_cur) {
        out[i] = -1; flag[i] = 0;
        if (!bad) mp_id[i] = -1;
    }
    if (bad && i < n_last) act[i] = 0;
}

// "Discard outliers" (src/Tracking.cpp:599-618), one thread per feature of the current frame: a feature that holds a point and is an
// outlier of the pose (outlier == nullptr: no pose ran, nothing is dropped) loses it; ids_out is the handle's copy for the download.
// head[1] counts the features that keep a point with observations: a wave's ballot, one atomic add per wave.
__global__ __launch_bounds__(TMM_TPB) void k_tmm_discard(int n, int* mp_id, const uint8_t* outlier, MptTable T, int* ids_out, int* head)
{
    const int i = blockIdx.x * TMM_TPB + threadIdx.x, lane = threadIdx.x & 63;
    bool counts = false;
    if (i < n) {
        int id = mp_id[i];
        if (id >= 0 && outlier && outlier[i]) { id = -1; mp_id[i] = -1; }
        ids_out[i] = id;
        counts = id >= 0 && id < T.capacity && (T.flags[id] & CCM_MP_HAS_OBS);
    }
    const unsigned long long ball = __ballot(counts);
    if (ball && lane == __ffsll((long long)ball) - 1) atomicAdd(head + 1, __popcll(ball));
}

// ---------------------------------------------------------------------------------------------------------------- launchers
void tmm_launch_project(hipStream_t s, const TmmArgs& A, const MptTable& T)
{
    if (A.n_last > 0) hipLaunchKernelGGL(k_tmm_project, dim3((A.n_last + TMM_TPB - 1) / TMM_TPB), dim3(TMM_TPB), 0, s, A, T);
}
void tmm_launch_clear(hipStream_t s, int n_cur, int n_last, const int* head, int* mp_id, int* out, uint8_t* flag, uint8_t* act)
{
    const int m = n_cur > n_last ? n_cur : n_last;
    if (m > 0) hipLaunchKernelGGL(k_tmm_clear, dim3((m + 255) / 256), dim3(256), 0, s, n_cur, n_last, head, mp_id, out, flag, act);
}
void tmm_launch_discard(hipStream_t s, int n, int* mp_id, const uint8_t* outlier, const MptTable& T, int* ids_out, int* head)
{
    if (n > 0) hipLaunchKernelGGL(k_tmm_discard, dim3((n + TMM_TPB - 1) / TMM_TPB), dim3(TMM_TPB), 0, s, n, mp_id, outlier, T, ids_out, head);
}
void mpt_launch_scatter(hipStream_t s, const MptTable& T, int n, const int* slot, const float* pos, const float* normal, const float* min_dist,
                        const float* max_dist, const uint8_t* desc, const uint8_t* flags)
{
    if (n > 0) hipLaunchKernelGGL(k_mpt_scatter, dim3((n + 255) / 256), dim3(256), 0, s, T, n, slot, pos, normal, min_dist, max_dist, desc, flags);
}
void mpt_launch_gather(hipStream_t s, const MptTable& T, int n, const int* slot, float* pos, float* normal, float* min_dist, float* max_dist,
                       uint8_t* desc, uint8_t* flags, int* seen)
{
    if (n > 0) hipLaunchKernelGGL(k_mpt_gather, dim3((n + 255) / 256), dim3(256), 0, s, T, n, slot, pos, normal, min_dist, max_dist, desc, flags, seen);
}
void slp_launch_mark(hipStream_t s, const MptTable& T, int n, const int* mp_id, int stamp, int* ids, uint8_t* occ, int* match, int* cnt)
{
    if (n > 0) hipLaunchKernelGGL(k_slp_mark, dim3((n + 255) / 256), dim3(256), 0, s, T, n, mp_id, stamp, ids, occ, match, cnt);
}
int slp_workgroups(int n_order) { return (n_order + SLP_TPB - 1) / SLP_TPB; }
void slp_launch_frustum(hipStream_t s, const SlpArgs& A, const MptTable& T, int* cnt)
{
    const int n_wg = slp_workgroups(A.n_order);
    if (n_wg > 0) hipLaunchKernelGGL(k_slp_frustum, dim3(n_wg), dim3(SLP_TPB), 0, s, A, T);
    hipLaunchKernelGGL(k_slp_scan, dim3(1), dim3(SCAN_TPB), 0, s, n_wg, A.wg_cnt, A.wg_off, cnt);
    if (n_wg > 0) hipLaunchKernelGGL(k_slp_compact, dim3(n_wg), dim3(SLP_TPB), 0, s, A, T);
}
void mpt_launch_refresh(hipStream_t s, const MptRefreshArgs& A, const MptTable& T)
{
    if (A.n > 0) hipLaunchKernelGGL(k_mpt_refresh, dim3((A.n + MPR_TPB / 64 - 1) / (MPR_TPB / 64)), dim3(MPR_TPB), 0, s, A, T);
}
void fuse_launch_project(hipStream_t s, const FuseArgs& A, const MptTable& T, int max_n)
{
    if (A.n_kf < 1 || A.n_points < 1) return;
    hipLaunchKernelGGL(k_fuse_where, dim3((A.n_points + 255) / 256), dim3(256), 0, s, A, T.capacity);
    if (max_n > 0) hipLaunchKernelGGL(k_fuse_held, dim3((max_n + 255) / 256, A.n_kf), dim3(256), 0, s, A, T.capacity);
    hipLaunchKernelGGL(k_fuse_project, dim3((A.n_points + FUSE_TPB - 1) / FUSE_TPB, A.n_kf), dim3(FUSE_TPB), 0, s, A, T);
}
void fuse_launch_membership(hipStream_t s, const FuseArgs& A, const MptTable& T, int max_n)
{
    if (A.n_points <= 0 || A.n_kf <= 0) return;
    hipLaunchKernelGGL(k_fuse_where, dim3((A.n_points + 255) / 256), dim3(256), 0, s, A, T.capacity);
    if (max_n > 0) hipLaunchKernelGGL(k_fuse_held, dim3((max_n + 255) / 256, A.n_kf), dim3(256), 0, s, A, T.capacity);
}
void fuse_launch_scatter(hipStream_t s, int nq, int n_pairs, const int* qpair, const int* sel_i, const int* sel_d, int* best_idx, int* best_dist)
{
    if (nq > 0) hipLaunchKernelGGL(k_fuse_scatter, dim3((nq + 255) / 256), dim3(256), 0, s, nq, n_pairs, qpair, sel_i, sel_d, best_idx, best_dist);
}
