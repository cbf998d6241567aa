// match_window.hip -- the windowed matchers: candidate lists per query (k_window_candidates), the per-query selection of Fuse /
// SearchBySim3 (k_window_select) and the order-dependent acceptance of SearchByProjection (k_window_greedy) (the other matcher
// files: match_types.h).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "match_types.h"
#include "match_device.h"

// Frame::GetFeaturesInArea (src/Frame.cpp:200-253) + the DescriptorDistance calls of the windowed matchers
// (SearchByProjection / Fuse / SearchBySim3 ..., cslam/src/ORBmatcher.cpp:71-148 and following): one wave per
// query walks the grid cells of its window in the reference's order (ix outer, iy inner, cell content in
// feature-index order), applies the level and |dx|,|dy| < r tests in float exactly as written there, and emits
// (feature index, Hamming distance) in that order through ballot compaction.
// BATCH: the queries of many keyframes in one launch, query q against grids[q_kf[q]]; the candidate indices are the keyframe's own.
template <bool BATCH>
__global__ __launch_bounds__(256) void k_window_candidates(WinGrid G1, const WinGrid* __restrict__ grids, const int* __restrict__ q_kf,
                                                           int nq, const float* __restrict__ qx, const float* __restrict__ qy,
                                                           const float* __restrict__ qr, const int* __restrict__ min_level,
                                                           const int* __restrict__ max_level, const uint8_t* __restrict__ qdesc, int cap,
                                                           int* __restrict__ cand_idx, int* __restrict__ cand_dist, int* __restrict__ cand_n)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= nq) return;
    const WinGrid G = BATCH ? grids[q_kf[q]] : G1;
    const float x = qx[q], y = qy[q], r = qr[q];
    const int minL = min_level[q], maxL = max_level[q];
    int n = 0;
    if (r >= 0.f) {                                        // r < 0 marks a query that is not searched
        const int nMinCellX = max(0, (int)floorf((x - G.min_x - r) * G.inv_w));
        const int nMaxCellX = min(G.cols - 1, (int)ceilf((x - G.min_x + r) * G.inv_w));
        const int nMinCellY = max(0, (int)floorf((y - G.min_y - r) * G.inv_h));
        const int nMaxCellY = min(G.rows - 1, (int)ceilf((y - G.min_y + r) * G.inv_h));
        if (nMinCellX < G.cols && nMaxCellX >= 0 && nMinCellY < G.rows && nMaxCellY >= 0) {
            const bool check = (minL > 0) || (maxL >= 0);
            const uint4* qd = reinterpret_cast<const uint4*>(qdesc) + 2 * (long long)q;
            const uint4 a0 = qd[0], a1 = qd[1];
            for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
                // the cells (ix, nMinCellY..nMaxCellY) are adjacent in the CSR (column-major grid): one contiguous item range
                const int k0 = G.cell_first[ix * G.rows + nMinCellY], k1 = G.cell_first[ix * G.rows + nMaxCellY + 1];
                for (int base = k0; base < k1; base += 64) {
                    const int k = base + lane;
                    bool keep = false; int i = 0;
                    if (k < k1) {
                        i = G.cell_items[k];
                        const int o = G.oct[i];
                        keep = !(check && (o < minL || (maxL >= 0 && o > maxL)));
                        const float dx = G.kx[i] - x, dy = G.ky[i] - y;
                        keep = keep && fabsf(dx) < r && fabsf(dy) < r;
                    }
                    const unsigned long long m = __ballot(keep);
                    if (keep) {
                        const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
                        if (pos < cap) {
                            const uint4* b = reinterpret_cast<const uint4*>(G.desc) + 2 * (long long)i;
                            cand_idx[(long long)q * cap + pos] = i;
                            cand_dist[(long long)q * cap + pos] = ham256(a0, a1, b[0], b[1]);
                        }
                    }
                    n += __popcll(m);
                }
            }
        }
    }
    if (lane == 0) cand_n[q] = n;
}
void match_launch_window(hipStream_t s, const WinGrid& G, int nq, const float* qx, const float* qy, const float* qr, const int* minl,
                         const int* maxl, const uint8_t* qdesc, int cap, int* ci, int* cd, int* cn)
{
    hipLaunchKernelGGL(k_window_candidates<false>, dim3((nq + 3) / 4), dim3(256), 0, s, G, (const WinGrid*)nullptr, (const int*)nullptr, nq, qx, qy, qr, minl, maxl, qdesc, cap,
                       ci, cd, cn);
}
void match_launch_window_batch(hipStream_t s, const WinGrid* grids, const int* q_kf, int nq, const float* qx, const float* qy, const float* qr, const int* minl,
                               const int* maxl, const uint8_t* qdesc, int cap, int* ci, int* cd, int* cn)
{
    if (nq > 0) hipLaunchKernelGGL(k_window_candidates<true>, dim3((nq + 3) / 4), dim3(256), 0, s, WinGrid{}, grids, q_kf, nq, qx, qy, qr, minl, maxl, qdesc, cap, ci, cd, cn);
}

// ---- device-side acceptance of the windowed matchers: no candidate list leaves the GPU.
// k_window_select: the selection loop of ORBmatcher::Fuse, both overloads (ORBmatcher.cpp:914-955, :1072-1100), and of
// SearchBySim3 (:1196-1245): the same window walk as k_window_candidates, but every lane keeps the best (distance, visiting
// position) of the candidates it filters and the wave reduces to ONE (index, distance) per query.  "First of equal distances
// wins" (the reference's strict `dist < bestDist` in visiting order) = minimum of distance * 2^32 + position.
// BATCH (ccm_fuse_select_batch): the queries of many keyframes in one launch; query q belongs to keyframe q_kf[q], whose grid is
// grids[q_kf[q]] (the server's fuse loops call Fuse once per neighbouring keyframe: src/Mapping.cpp:515-546, src/MapMerger.cpp:576-586).
template <bool BATCH>
__global__ __launch_bounds__(256) void k_window_select(WinGrid G1, const WinGrid* __restrict__ grids, const int* __restrict__ q_kf,
                                                       int nq, const float* __restrict__ qx, const float* __restrict__ qy,
                                                       const float* __restrict__ qr, const int* __restrict__ min_level,
                                                       const int* __restrict__ max_level, const uint8_t* __restrict__ qdesc,
                                                       const float* __restrict__ inv_sigma2, int accept_th,
                                                       int* __restrict__ best_idx, int* __restrict__ best_dist)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= nq) return;
    const WinGrid G = BATCH ? grids[q_kf[q]] : G1;
    const float x = qx[q], y = qy[q], r = qr[q];
    const int minL = min_level[q], maxL = max_level[q];
    unsigned long long best = ~0ull; int bidx = -1;
    int n = 0;
    if (r >= 0.f) {
        const int nMinCellX = max(0, (int)floorf((x - G.min_x - r) * G.inv_w));
        const int nMaxCellX = min(G.cols - 1, (int)ceilf((x - G.min_x + r) * G.inv_w));
        const int nMinCellY = max(0, (int)floorf((y - G.min_y - r) * G.inv_h));
        const int nMaxCellY = min(G.rows - 1, (int)ceilf((y - G.min_y + r) * G.inv_h));
        if (nMinCellX < G.cols && nMaxCellX >= 0 && nMinCellY < G.rows && nMaxCellY >= 0) {
            const uint4* qd = reinterpret_cast<const uint4*>(qdesc) + 2 * (long long)q;
            const uint4 a0 = qd[0], a1 = qd[1];
            for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
                const int k0 = G.cell_first[ix * G.rows + nMinCellY], k1 = G.cell_first[ix * G.rows + nMaxCellY + 1];
                for (int base = k0; base < k1; base += 64) {
                    const int k = base + lane;
                    bool in_window = false, keep = false; int i = 0;
                    if (k < k1) {
                        i = G.cell_items[k];
                        const float dx = G.kx[i] - x, dy = G.ky[i] - y;
                        in_window = fabsf(dx) < r && fabsf(dy) < r;           // GetFeaturesInArea is called without level limits here
                        const int o = G.oct[i];
                        keep = in_window && !(o < minL || o > maxL);           // :925-926 / :1081-1082 kpLevel in [level-1, level]
                        if (keep && inv_sigma2) {                              // :929-937: chi2 of the reprojection, Fuse(pKF, vpMapPoints) only
                            const float ex = x - G.kx[i], ey = y - G.ky[i];
                            const float e2 = ex * ex + ey * ey;
                            if ((double)(e2 * inv_sigma2[o]) > 5.99) keep = false;
                        }
                    }
                    const unsigned long long m = __ballot(in_window);
                    if (keep) {
                        const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
                        const uint4* b = reinterpret_cast<const uint4*>(G.desc) + 2 * (long long)i;
                        const unsigned long long key = ((unsigned long long)ham256(a0, a1, b[0], b[1]) << 32) | (unsigned)pos;
                        if (key < best) { best = key; bidx = i; }
                    }
                    n += __popcll(m);
                }
            }
        }
    }
    unsigned long long wbest = best;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(wbest, d, 64); wbest = o < wbest ? o : wbest; }
    const unsigned long long owner = __ballot(best == wbest && bidx >= 0);
    int idx = -1, dist = 256;
    if (owner) { idx = __shfl(bidx, __ffsll((long long)owner) - 1, 64); dist = (int)(wbest >> 32); }
    if (lane == 0) { best_dist[q] = dist; best_idx[q] = dist <= accept_th ? idx : -1; }
}
void match_launch_window_select(hipStream_t s, const WinGrid& G, int nq, const float* qx, const float* qy, const float* qr, const int* minl,
                                const int* maxl, const uint8_t* qdesc, const float* inv_sigma2, int accept_th, int* best_idx, int* best_dist)
{
    hipLaunchKernelGGL(k_window_select<false>, dim3((nq + 3) / 4), dim3(256), 0, s, G, (const WinGrid*)nullptr, (const int*)nullptr, nq, qx, qy, qr, minl, maxl, qdesc, inv_sigma2,
                       accept_th, best_idx, best_dist);
}
void match_launch_window_select_batch(hipStream_t s, const WinGrid* grids, const int* q_kf, int nq, const float* qx, const float* qy, const float* qr,
                                      const int* minl, const int* maxl, const uint8_t* qdesc, const float* inv_sigma2, int accept_th, int* best_idx, int* best_dist)
{
    if (nq > 0) hipLaunchKernelGGL(k_window_select<true>, dim3((nq + 3) / 4), dim3(256), 0, s, WinGrid{}, grids, q_kf, nq, qx, qy, qr, minl, maxl, qdesc, inv_sigma2,
                                   accept_th, best_idx, best_dist);
}

// k_window_greedy: the ORDER-DEPENDENT acceptance of SearchByProjection(Frame&, vpMapPoints) (ORBmatcher.cpp:71-148, MODE 0),
// SearchByProjection(pKF, Scw, vpPoints, vpMatched) (:308-446, MODE 1) and SearchByProjection(CurrentFrame, LastFrame / KeyFrame)
// (:1350-1476, :1478-1605, MODE 2) on the candidate lists k_window_candidates left in HBM.
// The reference visits the map points one after the other, and a point's choice depends on which features earlier points have
// taken (`occupied` / `vpMatched` / the frame's map-point slots).  A point takes the nearest of its still-free candidates (MODE 0
// also looks at the second nearest for the ratio test), and flags are only ever SET.  Hence the parallel form used here:
//   an unresolved point may decide as soon as NO EARLIER unresolved point has the feature it would take (MODE 0: the two it
//   looks at) among its own free candidates.  Flags that earlier points set later can then only fall on candidates this point
//   does not look at -- removing them changes neither its minimum nor the list order of the rest -- and the flag this point sets
//   falls on a feature no earlier unresolved point can choose.  "No acceptable candidate" is final at once: candidates only vanish.
// The earliest unresolved point always decides, so the rounds end.
// Layout: one workgroup of 16 waves; 1024 consecutive points per batch, thread = point, its first 16 candidates (feature | distance)
// in registers -- all global loads of a batch are issued by all threads at once; then the waves take turns in point order, and inside
// a wave the rounds need no workgroup barrier: claim[feature] = lowest lane among the unresolved lanes that have the feature free
// (LDS atomicMin), decide where the claim on the wanted feature(s) is one's own, reset the claims.  With many points per feature
// (20,000 points on a 1,000-feature keyframe) round 2's first version -- claims on ALL free candidates over the whole list, 48 rounds,
// then one wave visiting the rest in order with two global round trips per point -- took 9.1 ms; this takes the same decisions.
#define WG_REG_CAND 16
#define WG_BATCH_ROUNDS 3
template <int MODE>
__global__ __launch_bounds__(1024) void k_window_greedy(GreedyArgs A)
{
    if (A.kfs) {
        const GreedyKf k = A.kfs[blockIdx.x];
        A.ci += (long long)k.q0 * A.cap; A.cd += (long long)k.q0 * A.cap; A.cn += k.q0; A.active += k.q0; A.qflag += k.q0;
        if (A.qlevel) A.qlevel += k.q0;
        A.oct += k.f0; A.flag += k.f0; A.out += MODE == 1 ? k.q0 : k.f0; A.status += 3 * blockIdx.x;
        A.nq = k.nq; A.n = k.n;
    }
    extern __shared__ int wg_lds[];
    int* claim = wg_lds;                                            // [n]
    uint8_t* flag = reinterpret_cast<uint8_t*>(claim + A.n);        // [n]
    uint8_t* octl = flag + ((A.n + 3) & ~3);                        // [n] octave per feature
    __shared__ int s_count, s_maxcn, s_rounds;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) { s_count = 0; s_maxcn = 0; s_rounds = 0; }
    for (int i = tid; i < A.n; i += 1024) { flag[i] = A.flag[i]; octl[i] = (uint8_t)A.oct[i]; claim[i] = 0x7FFFFFFF; }
    __syncthreads();
    int mx = 0;
    for (int m = tid; m < A.nq; m += 1024) mx = max(mx, A.cn[m]);
    atomicMax(&s_maxcn, mx);
    __syncthreads();
    if (s_maxcn > A.cap) { if (tid == 0) { A.status[0] = -1; A.status[1] = s_maxcn; A.status[2] = 0; } return; }   // the host retries with longer lists
    int mine = 0, most = 0;
    for (int base = 0; base < A.nq; base += 1024) {
        const int m = base + tid;
        int c = 0, lvl = 0, qf = 0;
        unsigned cand[WG_REG_CAND];                                  // feature | distance << 16
        if (m < A.nq && A.active[m]) c = A.cn[m];
        const int* ci = A.ci + (long long)min(m, A.nq - 1) * A.cap; const int* cd = A.cd + (long long)min(m, A.nq - 1) * A.cap;
#pragma unroll
        for (int k = 0; k < WG_REG_CAND; k++) cand[k] = k < c ? ((unsigned)ci[k] | ((unsigned)cd[k] << 16)) : 0u;
        if (c > 0) { qf = A.qflag[m]; if (MODE == 1) lvl = A.qlevel[m]; }
        if (MODE == 2 && m < A.nq) A.ev[m] = -1;
        // candidate k of this point is free and of a level the point may take
        auto usable = [&](int idx) -> bool {
            if (flag[idx]) return false;
            if (MODE == 1) { const int kl = octl[idx]; if (kl < lvl - 1 || kl > lvl) return false; }      // :394-400
            return true;
        };
        // one claim round for the unresolved points: `me` orders them (thread id inside the batch, or lane inside a wave); WG selects
        // the workgroup barrier (all 1024 points at once) or the wave barrier (one wave on its turn)
        bool unres = c > 0;
        auto sync = [&](bool wg) {
            if (wg) __syncthreads();
            else { __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier(); }
        };
        auto round = [&](int me, bool wg) {
            // nearest and second nearest usable candidate in (distance, list position) order: what the sequential scan's
            // `dist < bestDist` / `else if dist < bestDist2` keeps; and the claims
            unsigned k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;
            if (unres) {
#pragma unroll
                for (int k = 0; k < WG_REG_CAND; k++) {
                    if (k < c) {
                        const int idx = (int)(cand[k] & 0xFFFFu);
                        if (usable(idx)) {
                            atomicMin(&claim[idx], me);
                            const unsigned key = (cand[k] & 0xFFFF0000u) | (unsigned)k;
                            if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
                        }
                    }
                }
                for (int k = WG_REG_CAND; k < c; k++) {
                    const int idx = ci[k];
                    if (usable(idx)) {
                        atomicMin(&claim[idx], me);
                        const unsigned key = ((unsigned)cd[k] << 16) | (unsigned)k;
                        if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
                    }
                }
            }
            sync(wg);
            const int th = MODE == 0 ? 100 : (MODE == 1 ? 50 : A.orb_dist);       // TH_HIGH / TH_LOW / TH_HIGH or ORBdist
            const int bestDist = k1 == 0xFFFFFFFFu ? 256 : (int)(k1 >> 16);
            int idx1 = -1, idx2 = -1;
            bool safe = false;
            if (unres) {
                if (bestDist > th) safe = true;                                     // no acceptable candidate: final
                else {
                    const int p1 = (int)(k1 & 0xFFFFu), p2 = (int)(k2 & 0xFFFFu);
                    if (p1 >= WG_REG_CAND) idx1 = ci[p1];
                    if (MODE == 0 && k2 != 0xFFFFFFFFu && p2 >= WG_REG_CAND) idx2 = ci[p2];
#pragma unroll
                    for (int k = 0; k < WG_REG_CAND; k++) {
                        if (k == p1) idx1 = (int)(cand[k] & 0xFFFFu);
                        if (MODE == 0 && k2 != 0xFFFFFFFFu && k == p2) idx2 = (int)(cand[k] & 0xFFFFu);
                    }
                    safe = claim[idx1] == me;
                    if (MODE == 0 && idx2 >= 0) safe = safe && claim[idx2] == me;
                }
            }
            sync(wg);
            if (unres) {                                                            // claims back to "nobody"
#pragma unroll
                for (int k = 0; k < WG_REG_CAND; k++) if (k < c) claim[cand[k] & 0xFFFFu] = 0x7FFFFFFF;
                for (int k = WG_REG_CAND; k < c; k++) claim[ci[k]] = 0x7FFFFFFF;
            }
            if (unres && safe) {
                unres = false;
                if (bestDist <= th) {
                    if (MODE == 0) {
                        const int bestLevel = octl[idx1], bestLevel2 = idx2 >= 0 ? (int)octl[idx2] : -1;
                        const int bestDist2 = idx2 >= 0 ? (int)(k2 >> 16) : 256;
                        if (!(bestLevel == bestLevel2 && bestDist > A.nnratio * bestDist2)) { A.out[idx1] = m; flag[idx1] = (uint8_t)qf; mine++; }
                    } else if (MODE == 1) {
                        A.out[m] = idx1;
                        if (!qf) { flag[idx1] = 1; mine++; }                        // :436-440
                    } else {
                        A.out[idx1] = m;
                        flag[idx1] = (uint8_t)qf;
                        int bin = 255;
                        if (A.check_ori) {                                          // :1437-1447
                            bin = rot_bin(A.q_angle[m] - A.f_angle[idx1]);
                        }
                        A.ev[m] = (idx1 << 8) | bin;
                        mine++;
                    }
                }
            }
        };
        // (1) a few rounds over the whole batch: with few points per feature nearly every point decides here
        int left = 1, rounds = 0;
        for (int r = 0; r < WG_BATCH_ROUNDS && left; r++) {
            round(tid, true);
            left = __syncthreads_count(unres ? 1 : 0);                              // also: flags and claim resets visible to all
            rounds++;
        }
        // (2) what is left (many points wanting the same features) is finished wave by wave, in point order, without workgroup barriers
        //     inside a wave's turn
        if (left) {
            for (int turn = 0; turn < 16; turn++) {
                if (wv == turn) {
                    while (__ballot(unres) != 0ull) {
                        rounds++;
                        round(lane, false);
                        __builtin_amdgcn_s_waitcnt(0xc07f);
                        __builtin_amdgcn_wave_barrier();
                    }
                }
                __syncthreads();
            }
        }
        most = max(most, rounds);
    }
    if (mine) atomicAdd(&s_count, mine);
    atomicMax(&s_rounds, most);
    __syncthreads();
    if (MODE == 2 && A.check_ori) {
        // rotation consistency (:1453-1471): histogram of the accepted matches' angle differences, the three largest bins stay
        // (ComputeThreeMaxima :1607-1648), every match recorded in another bin is cleared -- also when a later point re-took the feature
        __shared__ int hist[30], keep3[3], s_removed;
        if (tid < 30) hist[tid] = 0;
        if (tid == 0) s_removed = 0;
        __syncthreads();
        for (int m = tid; m < A.nq; m += 1024) { const int e = (A.active[m] && A.cn[m] > 0) ? A.ev[m] : -1; if (e >= 0) atomicAdd(&hist[e & 255], 1); }
        __syncthreads();
        if (tid == 0) {
            int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
            for (int i = 0; i < 30; i++) {
                const int sz = hist[i];
                if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; i3 = i2; i2 = i1; i1 = i; }
                else if (sz > max2) { max3 = max2; max2 = sz; i3 = i2; i2 = i; }
                else if (sz > max3) { max3 = sz; i3 = i; }
            }
            if (max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
            else if (max3 < 0.1f * (float)max1) { i3 = -1; }
            keep3[0] = i1; keep3[1] = i2; keep3[2] = i3;
        }
        __syncthreads();
        int removed = 0;
        for (int m = tid; m < A.nq; m += 1024) {
            const int e = (A.active[m] && A.cn[m] > 0) ? A.ev[m] : -1;
            if (e < 0) continue;
            const int b = e & 255;
            if (b != keep3[0] && b != keep3[1] && b != keep3[2]) { A.out[e >> 8] = -1; removed++; }
        }
        if (removed) atomicAdd(&s_removed, removed);
        __syncthreads();
        if (tid == 0) s_count -= s_removed;
        __syncthreads();
    }
    for (int i = tid; i < A.n; i += 1024) A.flag[i] = flag[i];
    if (tid == 0) { A.status[0] = s_count; A.status[1] = s_maxcn; A.status[2] = s_rounds; }
}
size_t match_window_greedy_lds(int n, int nq) { (void)nq; return (size_t)4 * n + 2 * (size_t)((n + 3) & ~3) + 16; }
// n_wg workgroups of k_window_greedy<MODE> with `lds` bytes of dynamic LDS; -1 when the runtime refuses that much
template <int MODE>
static int launch_window_greedy(hipStream_t s, const GreedyArgs& A, int n_wg, size_t lds)
{
    if (hipFuncSetAttribute((const void*)k_window_greedy<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_window_greedy<MODE>, dim3(n_wg), dim3(1024), lds, s, A);
    return 0;
}
int match_launch_window_greedy_batch(hipStream_t s, const GreedyArgs& A, int n_kf, int max_n)
{
    return launch_window_greedy<1>(s, A, n_kf, match_window_greedy_lds(max_n, 0));
}
int match_launch_window_greedy(hipStream_t s, int mode, const GreedyArgs& A)
{
    const size_t lds = match_window_greedy_lds(A.n, A.nq);
    return mode == 0 ? launch_window_greedy<0>(s, A, 1, lds) : mode == 1 ? launch_window_greedy<1>(s, A, 1, lds) : launch_window_greedy<2>(s, A, 1, lds);
}
