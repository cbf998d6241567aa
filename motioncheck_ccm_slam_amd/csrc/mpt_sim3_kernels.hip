// mpt_sim3_kernels.hip -- ComputeSim3's two matchers on keyframe handles and the map-point table (include/ccm_hot.h "ComputeSim3 on
// keyframe handles and the table"), gfx950:
//   k_sim3_marks / k_sim3_project / k_sim3_agree
//                      ccm_search_by_sim3_table_frames: the two projections and gates of ORBmatcher::SearchBySim3
//                      (src/ORBmatcher.cpp:1124-1348) and its agreement check; the selections are k_window_select's
//   k_loop_marks / k_loop_project / k_loop_finish
//                      ccm_search_by_projection_table_frames: the projection and gates of SearchByProjection(pKF, Scw, ...) (:308-446);
//                      the candidate lists and the order-dependent acceptance are k_window_candidates' and k_window_greedy's
// The projection arithmetic restates a few lines of k_fuse_project (mpt_kernels.hip) rather than share them: that kernel stays as it is.
// Float arithmetic of a float cv::Mat: the products of a matrix product, a dot and a norm are summed in double and stored as float;
// everything else is float, rounded per operation (built with -ffp-contract=off, and spelled out with __fmul_rn / __fadd_rn / __fdiv_rn).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/ccm_hot.h"
#include "mpt_types.h"
#include "match_types.h"
#include "match_device.h"

// MapPoint::PredictScale (src/MapPoint.cpp:837-852): the expression of fuse_predict_level (mpt_kernels.hip)
__device__ inline int sim3_predict_level(float max_d, float dist, float log_scale, int n_levels)
{
    const float ratio = max_d / dist;
    const float lg = (float)log((double)ratio);
    const float q = ceilf(lg / log_scale);
    return !(q >= 0.0f) ? 0 : (q >= (float)n_levels ? n_levels - 1 : (int)q);
}

// row-major [3][4] M times (P, 1): the sum in double, stored as float
__device__ inline void sim3_mat_point(const float* M, const float* P, float* out)
{
    for (int r = 0; r < 3; r++)
        out[r] = (float)((double)M[4 * r] * (double)P[0] + (double)M[4 * r + 1] * (double)P[1] + (double)M[4 * r + 2] * (double)P[2] + (double)M[4 * r + 3]);
}

// ---------------------------------------------------------------------------------------------------------------- SearchBySim3
// vbAlreadyMatched2 (:1154-1164): one thread per feature of side 1; several features naming one index write the same value
__global__ void k_sim3_marks(const Sim3Pair* pairs, const int* matched12, const int* matched_idx2, uint8_t* am2)
{
    const Sim3Pair P = pairs[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n1) return;
    if (matched12[P.first1 + i] < 0) return;
    const int i2 = matched_idx2[P.first1 + i];
    if (i2 >= 0 && i2 < P.n2) am2[P.first2 + i2] = 1;                // :1161
}

// One thread per (pair, direction, feature); blockIdx.y = 2 * pair + direction, so the view is the same for the whole workgroup and
// is read through scalar loads.  The survivors of a wave take consecutive places of the query list behind ONE atomic add, as in
// k_fuse_project; the order of the list is free: k_window_select decides per query and the scatter writes by entry.
__global__ __launch_bounds__(SIM3_TPB) void k_sim3_project(Sim3Args A, MptTable T)
{
    const int i = blockIdx.x * SIM3_TPB + threadIdx.x, k = blockIdx.y, lane = threadIdx.x & 63;
    const Sim3View& V = A.views[k];
    const int e = V.e0 + (i < V.n ? i : 0);
    bool keep = false;
    int gate = CCM_SG_NO_POINT, level = 0, s = -1;
    float u = 0.0f, v = 0.0f;
    if (i < V.n) {
        s = V.mp_id[i];
        uint8_t fl = 0;
        if (s >= 0 && s < T.capacity) fl = T.flags[s];
        if (fl & CCM_MP_LIVE) {
            gate = CCM_SG_MATCHED;
            if (!(V.mark_i ? V.mark_i[i] >= 0 : V.mark_b[i] != 0)) {
                gate = CCM_SG_BAD;
                if (!(fl & CCM_MP_BAD)) {
                    const float P[3] = { T.pos[3 * (size_t)s], T.pos[3 * (size_t)s + 1], T.pos[3 * (size_t)s + 2] };
                    float Ps[3], Pt[3];
                    sim3_mat_point(V.Tsw, P, Ps);                    // :1181 / :1261
                    sim3_mat_point(V.Sts, Ps, Pt);                   // :1182 / :1262
                    gate = CCM_SG_BEHIND;
                    if (!(Pt[2] < 0.0f)) {
                        const float invz = __fdiv_rn(1.0f, Pt[2]);
                        const float x = __fmul_rn(Pt[0], invz), y = __fmul_rn(Pt[1], invz);
                        u = __fadd_rn(__fmul_rn(V.fx, x), V.cx);
                        v = __fadd_rn(__fmul_rn(V.fy, y), V.cy);
                        gate = CCM_SG_OUTSIDE;
                        if (u >= V.min_x && u < V.max_x && v >= V.min_y && v < V.max_y) {      // KeyFrame::IsInImage; a NaN is outside
                            const float max_d = T.max_dist[s];
                            const float dist = (float)sqrt((double)Pt[0] * (double)Pt[0] + (double)Pt[1] * (double)Pt[1] + (double)Pt[2] * (double)Pt[2]);
                            gate = CCM_SG_DISTANCE;
                            if (!(dist < 0.8f * T.min_dist[s] || dist > 1.2f * max_d)) {
                                level = sim3_predict_level(max_d, dist, A.log_scale[V.side_t], A.n_levels[V.side_t]);
                                gate = V.n_target > 0 ? CCM_SG_SEARCHED : CCM_SG_EMPTY_KF;
                                keep = V.n_target > 0;
                            }
                        }
                    }
                }
            }
        }
        A.sel[e] = -1;
        if (A.gate) A.gate[e] = (uint8_t)gate;
        if (A.u) { A.u[e] = u; A.v[e] = v; A.level[e] = level; }
    }
    const unsigned long long ball = __ballot(keep);
    if (!ball) return;
    const int leader = __ffsll((long long)ball) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(A.cnt, __popcll(ball));
    base = __shfl(base, leader, 64);
    if (!keep) return;
    const int q = base + __popcll(ball & ((1ull << lane) - 1ull));
    if (q < 0 || q >= A.n_entries) return;       // cannot happen: at most one query per entry
    A.qx[q] = u; A.qy[q] = v; A.qr[q] = A.th * A.scale[V.side_t][level];     // :1211 / :1291
    A.minl[q] = level - 1; A.maxl[q] = level;                                // :1229 / :1309
    A.qview[q] = k; A.qent[q] = e;
    const uint4* a = reinterpret_cast<const uint4*>(T.desc + (size_t)s * 32);
    uint4* b = reinterpret_cast<uint4*>(A.qdesc + (size_t)q * 32);
    b[0] = a[0]; b[1] = a[1];
}

// The agreement check (:1330-1345): one thread per feature of side 1
__global__ void k_sim3_agree(const Sim3Pair* pairs, const int* sel, int n_side1, int* match12)
{
    const Sim3Pair P = pairs[blockIdx.y];
    const int i1 = blockIdx.x * blockDim.x + threadIdx.x;
    if (i1 >= P.n1) return;
    const int i2 = sel[P.first1 + i1];
    int m = -1;
    if (i2 >= 0 && i2 < P.n2 && sel[n_side1 + P.first2 + i2] == i1) m = i2;
    match12[P.first1 + i1] = m;
}

// ---------------------------------------------------------------------------------------------------------------- SearchByProjection(Scw)
// Per (view, feature): the vpMatched flag, the octave (k_window_greedy reads the views' features from one array) and the copy of
// matched_slot the call returns; spAlreadyFound (:324) by the stamped where[] of k_fuse_where: the slot's position in this call's list.
__global__ void k_loop_marks(int n_points, const WinGrid* grids, const int* feat_first, const int* matched_slot, const unsigned long long* where,
                             unsigned stamp, int capacity, uint8_t* flag, int* oct, int* ms_out, uint8_t* found)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    const WinGrid& G = grids[k];
    if (i >= G.n) return;
    const int f = feat_first[k] + i;
    const int s = matched_slot[f];
    flag[f] = s >= 0 ? 1 : 0;
    oct[f] = G.oct[i];
    ms_out[f] = s;
    if (s < 0 || s >= capacity) return;          // a slot outside the table names none of the listed points
    const unsigned long long w = where[s];
    const unsigned pos = (unsigned)w;
    if ((unsigned)(w >> 32) == stamp && pos < (unsigned)n_points) found[(size_t)k * n_points + pos] = 1;
}

// One thread per (view, point); blockIdx.y = the view.  The queries stay in list order, one per pair: the acceptance depends on it.
__global__ __launch_bounds__(LOOP_TPB) void k_loop_project(LoopArgs A, MptTable T)
{
    const int j = blockIdx.x * LOOP_TPB + threadIdx.x, k = blockIdx.y;
    if (j >= A.n_points) return;
    const FuseView& V = A.views[k];
    const size_t pair = (size_t)k * A.n_points + j;
    int gate = CCM_LG_SKIPPED, level = 0;
    float u = 0.0f, v = 0.0f;
    const int s = A.slot[j];
    uint8_t fl = 0;
    if (s >= 0 && s < T.capacity) fl = T.flags[s];
    if ((fl & CCM_MP_LIVE) && !(fl & CCM_MP_BAD)) {
        gate = CCM_LG_ALREADY_FOUND;
        if (!A.found[pair]) {
            const float P[3] = { T.pos[3 * (size_t)s], T.pos[3 * (size_t)s + 1], T.pos[3 * (size_t)s + 2] };
            float Pc[3];
            sim3_mat_point(V.Tcw, P, Pc);                            // :342
            gate = CCM_LG_BEHIND;
            if (!(Pc[2] < 0.0f)) {
                const float invz = __fdiv_rn(1.0f, Pc[2]);
                const float x = __fmul_rn(Pc[0], invz), y = __fmul_rn(Pc[1], invz);
                u = __fadd_rn(__fmul_rn(V.fx, x), V.cx);
                v = __fadd_rn(__fmul_rn(V.fy, y), V.cy);
                gate = CCM_LG_OUTSIDE;
                if (u >= V.min_x && u < V.max_x && v >= V.min_y && v < V.max_y) {
                    const float max_d = T.max_dist[s];
                    const float PO[3] = { P[0] - V.Ow[0], P[1] - V.Ow[1], P[2] - V.Ow[2] };
                    const float dist = (float)sqrt((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1] + (double)PO[2] * (double)PO[2]);
                    gate = CCM_LG_DISTANCE;
                    if (!(dist < 0.8f * T.min_dist[s] || dist > 1.2f * max_d)) {
                        const double dot = (double)PO[0] * (double)T.normal[3 * (size_t)s] + (double)PO[1] * (double)T.normal[3 * (size_t)s + 1] +
                                           (double)PO[2] * (double)T.normal[3 * (size_t)s + 2];
                        gate = CCM_LG_ANGLE;
                        if (!(dot < 0.5 * (double)dist)) {
                            level = sim3_predict_level(max_d, dist, A.log_scale, A.n_levels);
                            gate = V.n > 0 ? CCM_LG_SEARCHED : CCM_LG_EMPTY_KF;
                        }
                    }
                }
            }
        }
    }
    const bool on = gate == CCM_LG_SEARCHED;
    A.qx[pair] = u; A.qy[pair] = v; A.qr[pair] = on ? A.th * A.scale[level] : -1.0f;      // :378
    A.none[pair] = -1; A.qkf[pair] = k; A.qlevel[pair] = level; A.act[pair] = on ? 1 : 0;
    A.out[pair] = -1;
    uint4* b = reinterpret_cast<uint4*>(A.qdesc + pair * 32);
    if (on) {
        const uint4* a = reinterpret_cast<const uint4*>(T.desc + (size_t)s * 32);
        b[0] = a[0]; b[1] = a[1];
    } else {
        b[0] = make_uint4(0, 0, 0, 0); b[1] = make_uint4(0, 0, 0, 0);
    }
    if (A.gate) A.gate[pair] = (uint8_t)gate;
    if (A.u) { A.u[pair] = u; A.v[pair] = v; A.level[pair] = level; }
}

// After the acceptance: vpMatched[bestIdx] = pMP for the accepted points the keyframe does not observe (:439) -- the acceptance gave
// each of them a feature of its own -- and the optional distance tap
__global__ void k_loop_finish(int n_points, const WinGrid* grids, const int* feat_first, const int* slot, const int* out, const uint8_t* held,
                              MptTable T, int* ms_out, int* best_dist)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (j >= n_points) return;
    const WinGrid& G = grids[k];
    const size_t pair = (size_t)k * n_points + j;
    const int bi = out[pair], s = slot[j];
    const bool ok = bi >= 0 && bi < G.n && s >= 0 && s < T.capacity;
    if (ok && !held[pair]) ms_out[feat_first[k] + bi] = s;
    if (best_dist) {
        int d = 256;
        if (ok) {
            const uint4* a = reinterpret_cast<const uint4*>(T.desc + (size_t)s * 32);
            const uint4* b = reinterpret_cast<const uint4*>(G.desc) + 2 * (size_t)bi;
            d = ham256(a[0], a[1], b[0], b[1]);
        }
        best_dist[pair] = d;
    }
}

// ---------------------------------------------------------------------------------------------------------------- launchers
void sim3_launch_marks(hipStream_t s, int n_pairs, int max_n1, const Sim3Pair* pairs, const int* matched12, const int* matched_idx2, uint8_t* am2)
{
    if (n_pairs > 0 && max_n1 > 0) hipLaunchKernelGGL(k_sim3_marks, dim3((max_n1 + 255) / 256, n_pairs), dim3(256), 0, s, pairs, matched12, matched_idx2, am2);
}
void sim3_launch_project(hipStream_t s, const Sim3Args& A, const MptTable& T, int max_n)
{
    if (A.n_views > 0 && max_n > 0) hipLaunchKernelGGL(k_sim3_project, dim3((max_n + SIM3_TPB - 1) / SIM3_TPB, A.n_views), dim3(SIM3_TPB), 0, s, A, T);
}
void sim3_launch_agree(hipStream_t s, int n_pairs, int max_n1, const Sim3Pair* pairs, const int* sel, int n_side1, int* match12)
{
    if (n_pairs > 0 && max_n1 > 0) hipLaunchKernelGGL(k_sim3_agree, dim3((max_n1 + 255) / 256, n_pairs), dim3(256), 0, s, pairs, sel, n_side1, match12);
}
void loop_launch_marks(hipStream_t s, int n_kf, int n_points, int max_n, const WinGrid* grids, const int* feat_first, const int* matched_slot,
                       const unsigned long long* where, unsigned stamp, int capacity, uint8_t* flag, int* oct, int* ms_out, uint8_t* found)
{
    if (n_kf > 0 && max_n > 0)
        hipLaunchKernelGGL(k_loop_marks, dim3((max_n + 255) / 256, n_kf), dim3(256), 0, s, n_points, grids, feat_first, matched_slot, where, stamp, capacity,
                           flag, oct, ms_out, found);
}
void loop_launch_project(hipStream_t s, const LoopArgs& A, const MptTable& T)
{
    if (A.n_kf > 0 && A.n_points > 0) hipLaunchKernelGGL(k_loop_project, dim3((A.n_points + LOOP_TPB - 1) / LOOP_TPB, A.n_kf), dim3(LOOP_TPB), 0, s, A, T);
}
void loop_launch_finish(hipStream_t s, int n_kf, int n_points, const WinGrid* grids, const int* feat_first, const int* slot, const int* out,
                        const uint8_t* held, const MptTable& T, int* ms_out, int* best_dist)
{
    if (n_kf > 0 && n_points > 0)
        hipLaunchKernelGGL(k_loop_finish, dim3((n_points + 255) / 256, n_kf), dim3(256), 0, s, n_points, grids, feat_first, slot, out, held, T, ms_out, best_dist);
}
