// match_bf.hip -- the Hamming kernels: brute-force best / second-best per query (k_hamming_mfma on the matrix cores, k_hamming_bf and
// k_hamming_merge on the vector ALU beyond HM_MAX_NT train rows), the known-answer tap k_fp4_tile, and k_hamming_ranges, distances
// only (the other matcher files: match_types.h).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "match_types.h"
#include "match_device.h"

#define BF_TILE 1024          // train descriptors staged per pass: 32 KiB of LDS
#define BF_THREADS 512        // (256 threads x 4 queries and 1024 x 1 were measured and lost)
#define BF_QPL 2              // queries per lane

// One workgroup per (pair, train split); a lane owns BF_QPL queries (8 VGPRs each); the train
// descriptors are staged in LDS once per 1024 and read back as wave-uniform (broadcast) b128 loads.
// Running state per query: best = (dist << 16 | index) so that v_min_u32 keeps the LOWEST index among
// equal distances, which is what the reference's strict `<` scan in index order keeps; second =
// min(second, max(dist, best_dist_before)), identical to its if / else-if.
// With n_split > 1 the train rows of a pair are divided over n_split workgroups that write partial
// (best, second) to scratch; k_hamming_merge combines them exactly (see there).
__global__ __launch_bounds__(BF_THREADS) void k_hamming_bf(
    const uint8_t* __restrict__ q, long long q_pair_bytes, const uint8_t* __restrict__ t, long long t_pair_bytes,
    int nq, int nt, const int* __restrict__ nq_n, const int* __restrict__ nt_n, int n_split,
    unsigned* __restrict__ part_best, int* __restrict__ part_second,
    int* __restrict__ best_idx, int* __restrict__ best_dist, int* __restrict__ second_dist)
{
    __shared__ uint4 tile[BF_TILE * 2];
    const int pair = blockIdx.x / n_split, split = blockIdx.x - pair * n_split, tid = threadIdx.x;
    const int nqp = nq_n ? min(max(nq_n[pair], 0), nq) : nq;
    const int ntp = nt_n ? min(max(nt_n[pair], 0), nt) : nt;
    // this workgroup's train rows [t_lo, t_hi): equal chunks rounded up to the wave-friendly 64
    const int chunk = ((ntp + n_split - 1) / n_split + 63) & ~63;
    const int t_lo = min(split * chunk, ntp), t_hi = min(t_lo + chunk, ntp);
    const uint4* qp = reinterpret_cast<const uint4*>(q + (long long)pair * q_pair_bytes);
    const uint4* tp = reinterpret_cast<const uint4*>(t + (long long)pair * t_pair_bytes);
    // rows past the live count only get the "no match" defaults (no train scan for them)
    const int q_done = ((nqp + BF_QPL * BF_THREADS - 1) / (BF_QPL * BF_THREADS)) * (BF_QPL * BF_THREADS);
    if (n_split == 1 || split == 0)
        for (int qi = q_done + tid; qi < nq; qi += BF_THREADS) {
            if (n_split > 1) {
                for (int sp = 0; sp < n_split; sp++) {
                    const long long o = ((long long)pair * n_split + sp) * nq + qi;
                    part_best[o] = (256u << 16) | 0xFFFFu; part_second[o] = 256;
                }
            } else {
                const long long o = (long long)pair * nq + qi;
                best_idx[o] = -1; best_dist[o] = 256; second_dist[o] = 256;
            }
        }
    for (int qbase = 0; qbase < nqp; qbase += BF_QPL * BF_THREADS) {
        uint4 a0[BF_QPL], a1[BF_QPL];
        unsigned best[BF_QPL]; int sec[BF_QPL];
#pragma unroll
        for (int k = 0; k < BF_QPL; k++) {
            const int qi = qbase + k * BF_THREADS + tid;
            a0[k] = make_uint4(0, 0, 0, 0); a1[k] = a0[k];
            if (qi < nqp) { a0[k] = qp[2 * qi]; a1[k] = qp[2 * qi + 1]; }
            best[k] = (256u << 16) | 0xFFFFu; sec[k] = 256;
        }
        for (int tbase = t_lo; tbase < t_hi; tbase += BF_TILE) {
            const int cnt = min(BF_TILE, t_hi - tbase);
            __syncthreads();
            for (int i = tid; i < 2 * cnt; i += BF_THREADS) tile[i] = tp[2 * tbase + i];
            __syncthreads();
#pragma unroll 2
            for (int j = 0; j < cnt; j++) {
                const uint4 b0 = tile[2 * j], b1 = tile[2 * j + 1];
                const unsigned idx = (unsigned)(tbase + j);
#pragma unroll
                for (int k = 0; k < BF_QPL; k++) {
                    const int d = ham256(a0[k], a1[k], b0, b1);
                    sec[k] = min(sec[k], max(d, (int)(best[k] >> 16)));
                    best[k] = min(best[k], ((unsigned)d << 16) | idx);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < BF_QPL; k++) {
            const int qi = qbase + k * BF_THREADS + tid;
            if (qi >= nq) continue;
            if (n_split > 1) {
                const long long o = ((long long)pair * n_split + split) * nq + qi;
                part_best[o] = best[k]; part_second[o] = sec[k];
            } else {
                const bool live = qi < nqp;
                const long long o = (long long)pair * nq + qi;
                best_idx[o] = (live && (best[k] >> 16) < 256u) ? (int)(best[k] & 0xFFFFu) : -1;
                best_dist[o] = live ? (int)(best[k] >> 16) : 256;
                second_dist[o] = live ? sec[k] : 256;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_hamming_mfma: the same best / second-best search on the matrix cores.
//   hamming(a, b) = popc(a) + popc(b) - 2 <a, b>   with <a, b> the dot product of the 0/1 bit vectors,
// so a 32 x 32 block of distances is a 32 x 32 x 256 matrix product on operands whose bits are expanded to numbers the matrix
// cores take, scaled so that a common bit adds -4096 = -(2 << 11) to the accumulator.  The product is four
// v_mfma_scale_f32_32x32x64_f8f6f4 per tile on FP4 operands.  A bit becomes an e2m1 nibble: train rows 0 / +1.0 (0b0010), query
// columns 0 / -1.0 (0b1010), both with the E8M0 block scale 2^6 (byte 133).  The accumulator is f32; every key below is an integer
// under 2^24 and every product a multiple of 4096, so every partial sum is exact in whatever order the hardware adds.  (An int8
// form, eight v_mfma_i32_32x32x32_i8 per tile, took twice the matrix-core cycles, operand registers and LDS: DESIGN.md section 4.)
// Layout: A operand = 32 train rows, B operand = 32 query columns.  C/D puts column j = lane & 31 on the lane and
// rows (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) in its 16 registers, i.e. a lane sees ONE query and 16 trains per
// tile, so the running (best, second) of that query are two registers per lane.  The accumulator of the first k-step
// is preloaded (C operand) with the row word ((popc(train) + HM_BIAS) << 11) | train index, so the matrix cores
// deliver the finished key
//   ((popc(train) - 2 <a, b> + HM_BIAS) << 11) | train index
// -- popc(query) is constant per lane and added at the end -- and the fold is  second = med3(best, second, key);
// best = min(best, key): two VALU instructions per distance instead of ~18, the rest is MFMA.
// A/B fragments: lane (h = lane >> 5, r = lane & 31) supplies to k-step s the bits [128 h + 32 s, 128 h + 32 s + 32) of its row /
// column as 32 nibbles; A and B use the same k assignment, which is all the dot product needs.
// One workgroup = 4 waves x 64 queries; the train fragments of a 32-train tile (4 KiB) are expanded once per workgroup into LDS
// (double-buffered) and read back as ds_read_b128.
typedef int hm_v4i __attribute__((ext_vector_type(4)));
typedef int hm_v8i __attribute__((ext_vector_type(8)));
typedef float hm_v4f __attribute__((ext_vector_type(4)));
typedef float hm_v16f __attribute__((ext_vector_type(16)));
// Launch geometry, measured (ms per launch at 255 pairs / at 10 k pairs, 1000 x 1000 descriptors per pair):
//   (CB 2, 4 workgroups per CU) 0.048 / 1.49;  (CB 2, 5 per CU: 93 registers) 0.048 / 1.50;  (CB 1, 8 per CU: 59 registers) 0.059 / 1.86;
//   (CB 2, 6 per CU) spills.  More resident waves buy nothing.
#define HM_CB 2                  // 32-query column blocks per wave
#define HM_WAVES 4
// HM_TT: 32-train tiles staged per barrier ("group"); 2 bought nothing, 4 (2 workgroups per CU) lost (measured on the former int8 form).
// It is settled at 1, and the group / sub-tile level it leaves in fetch, stage and the main loop is dead weight.  It stays only because
// folding it away moves one ds_read_b128 of the shipped kernel, i.e. the code would no longer be instruction for instruction what was measured.
#define HM_TT 1
#define HM_WG_PER_CU 4
#define HM_QW (32 * HM_CB)       // queries per wave
#define HM_TPB (64 * HM_WAVES)
#define HM_MAX_NT 2048           // train rows whose row words fit the LDS table (the launcher falls back beyond)
#define HM_BIAS 4352
#define HM_IDX_BITS 11           // train index field of a key (HM_MAX_NT = 2048 rows)
#define HM_SCALE 0x85858585      // E8M0 2^(133 - 127) = 64 in every byte: +1.0 * 64 * -1.0 * 64 = -(2 << HM_IDX_BITS)

#define HM_KS 4                  // k-steps (matrix instructions) per tile
// the key of "no train": 2^24, larger than every real key ((256 + HM_BIAS) << 11 | 2047 < 2^24) and never modified, because the
// fragments of rows past the live count are zero
#define HM_SENT 16777216.0f

// median of three keys (floats)
__device__ __forceinline__ float hm_med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }
// the smaller of two keys: positive floats, so min(a, b) = med3(a, b, 0) -- one v_med3_f32 with an inline constant
__device__ __forceinline__ float hm_min(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, 0.0f); }

// 8 bits -> 8 e2m1 nibbles: bit i goes to bit 4 i in three mask-and-shift steps, then times `one`: 2 = 0b0010 = +1.0 (trains),
// 10 = 0b1010 = -1.0 (queries)
__device__ __forceinline__ int hm_nibbles8(unsigned b, unsigned one)
{
    unsigned x = (b | (b << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    return (int)(x * one);
}
__device__ __forceinline__ hm_v4i hm_expand32_fp4(unsigned w, unsigned one)
{
    hm_v4i v;
    v.x = hm_nibbles8(w & 255u, one); v.y = hm_nibbles8((w >> 8) & 255u, one);
    v.z = hm_nibbles8((w >> 16) & 255u, one); v.w = hm_nibbles8(w >> 24, one);
    return v;
}
// one k-step of a tile: acc = A x B + c
__device__ __forceinline__ hm_v16f hm_mfma(const hm_v4i& a, const hm_v4i& b, const hm_v16f& c)
{
    // cbsz 4 / blgp 4: both operands FP4 (the low four of the eight operand registers)
    const hm_v8i a8 = { a.x, a.y, a.z, a.w, 0, 0, 0, 0 }, b8 = { b.x, b.y, b.z, b.w, 0, 0, 0, 0 };
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, c, 4, 4, 0, (int)HM_SCALE, 0, (int)HM_SCALE);
}

// 4 workgroups per CU (<= 128 registers per lane): 255 pairs x 4 live query blocks = 1020 workgroups fit in ONE round.
// The template parameter is unused.  It keeps the kernel (and its lambdas) an instantiation: with the linkage of a plain kernel the
// compiler orders the instructions of the staging block differently, and the measured code is the instantiation's
// (profiles/match_split_kernel_diff.txt).
template <int = 0>
__global__ __launch_bounds__(HM_TPB, HM_WG_PER_CU * HM_TPB / 256) void k_hamming_mfma(
    const uint8_t* __restrict__ q, long long q_pair_bytes, const uint8_t* __restrict__ t, long long t_pair_bytes,
    int nq, int nt, const int* __restrict__ nq_n, const int* __restrict__ nt_n, int q_blocks,
    int* __restrict__ best_idx, int* __restrict__ best_dist, int* __restrict__ second_dist)
{
    __shared__ hm_v4i frag[2][HM_TT * HM_KS][64];  // [buffer][sub-tile, k-step][lane]: 32 expanded nibbles
    __shared__ __attribute__((aligned(16))) float wall[HM_MAX_NT];   // per train: (popc + HM_BIAS) << 11 | index, the sentinel past the live count
    const int pair = blockIdx.x / q_blocks, qblk = blockIdx.x - pair * q_blocks;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5, r = lane & 31;
    const int nqp = nq_n ? min(max(nq_n[pair], 0), nq) : nq;
    const int ntp = nt_n ? min(max(nt_n[pair], 0), nt) : nt;
    const unsigned* qp = reinterpret_cast<const unsigned*>(q + (long long)pair * q_pair_bytes);
    const unsigned* tp = reinterpret_cast<const unsigned*>(t + (long long)pair * t_pair_bytes);
    const int q0 = qblk * (HM_QW * HM_WAVES) + wv * HM_QW;                    // this wave's first query
    if (qblk * (HM_QW * HM_WAVES) >= nqp) {                                 // whole block past the live queries: defaults only
        for (int i = tid; i < HM_QW * HM_WAVES; i += HM_TPB) {
            const int qi = qblk * (HM_QW * HM_WAVES) + i;
            if (qi < nq) { const long long o = (long long)pair * nq + qi; best_idx[o] = -1; best_dist[o] = 256; second_dist[o] = 256; }
        }
        return;
    }

    // ---- B fragments of the wave's queries (0 / -1.0 nibbles) and their popcounts, kept in registers
    hm_v4i bq[HM_CB][HM_KS];
    int pa[HM_CB];
#pragma unroll
    for (int cb = 0; cb < HM_CB; cb++) {
        const int qi = q0 + 32 * cb + r;
        // the lane's half of the row is all it expands; the other half's popcount comes from the partner lane
        const uint4 d = qi < nqp ? reinterpret_cast<const uint4*>(qp + 8 * (long long)qi)[h] : make_uint4(0, 0, 0, 0);
        const int pc = __popc(d.x) + __popc(d.y) + __popc(d.z) + __popc(d.w);
        pa[cb] = pc + __shfl_xor(pc, 32, 64);
        bq[cb][0] = hm_expand32_fp4(d.x, 10u); bq[cb][1] = hm_expand32_fp4(d.y, 10u);
        bq[cb][2] = hm_expand32_fp4(d.z, 10u); bq[cb][3] = hm_expand32_fp4(d.w, 10u);
    }
    float m1[HM_CB], m2[HM_CB];
#pragma unroll
    for (int cb = 0; cb < HM_CB; cb++) { m1[cb] = HM_SENT; m2[cb] = HM_SENT; }

    // ---- staging of one 32-train tile.  The raw words are fetched one tile ahead (issued before the MFMAs of the current tile) so
    //      that no wave waits on a global load.  A tile has FR fragments of 16 bytes; thread t owns fragments t, t + HM_TPB, ...
    //      Fragment f = dword f >> 5 of train f & 31, all of it: k-step (f >> 5) & 3 of lane half f >> 7 (one per thread and tile)
    // HM_TT tiles are staged per barrier ("group")
    constexpr int FR = 64 * HM_KS, HM_FPT = (FR * HM_TT + HM_TPB - 1) / HM_TPB;
    struct Raw { unsigned v[HM_FPT]; };
    auto fetch = [&](int group) {
        Raw x;
#pragma unroll
        for (int j = 0; j < HM_FPT; j++) {
            const int fi = tid + j * HM_TPB, sub = fi / FR, fw = fi % FR;
            const int tr = (group * HM_TT + sub) * 32 + (fw & 31);
            x.v[j] = (fi < FR * HM_TT && tr < ntp) ? tp[8 * (long long)tr + ((fw >> 5) & 7)] : 0u;
        }
        return x;
    };
    auto stage = [&](const Raw& x, int buf) {
#pragma unroll
        for (int j = 0; j < HM_FPT; j++) {
            const int fi = tid + j * HM_TPB, sub = fi / FR, fw = fi % FR;
            if (fi >= FR * HM_TT) continue;
            frag[buf][HM_KS * sub + ((fw >> 5) & 3)][32 * (fw >> 7) + (fw & 31)] = hm_expand32_fp4(x.v[j], 2u);
        }
    };
    // row words of all trains, once per workgroup
    for (int tr = tid; tr < ((ntp + 31) & ~31); tr += HM_TPB) {
        float w = HM_SENT;
        if (tr < ntp) {
            const uint4* d = reinterpret_cast<const uint4*>(tp + 8 * (long long)tr);
            const uint4 d0 = d[0], d1 = d[1];
            const int pb = __popc(d0.x) + __popc(d0.y) + __popc(d0.z) + __popc(d0.w) + __popc(d1.x) + __popc(d1.y) + __popc(d1.z) + __popc(d1.w);
            w = (float)(((pb + HM_BIAS) << HM_IDX_BITS) | tr);           // (below 2^24, the conversion is exact)
        }
        wall[tr] = w;
    }
    const int ntiles = (ntp + 31) >> 5;
    const bool wave_live = q0 < nqp;                                    // waves past the live queries only help staging
    // the matrix instructions of one tile into `acc`.  The accumulators start from the row words of the tile
    // (C operand of the first k-step: row = train, the same word in every query column), so what comes out IS the key
    //   ((popc(train) + HM_BIAS) << 11 | train) - (2 << 11) <train, query>.
    auto mma = [&](int tile, int buf, int sub, hm_v16f (&acc)[HM_CB]) {
        hm_v16f wc;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const hm_v4f w4 = *reinterpret_cast<const hm_v4f*>(&wall[32 * tile + 8 * g + 4 * h]);
            wc[4 * g] = w4.x; wc[4 * g + 1] = w4.y; wc[4 * g + 2] = w4.z; wc[4 * g + 3] = w4.w;
        }
#pragma unroll
        for (int s = 0; s < HM_KS; s++) {
            const hm_v4i a = frag[buf][HM_KS * sub + s][lane];
#pragma unroll
            for (int cb = 0; cb < HM_CB; cb++) acc[cb] = hm_mfma(a, bq[cb][s], s == 0 ? wc : acc[cb]);
        }
    };
    // (best, second) of the lane's query folded over the 16 keys it sees in `acc`: v_med3_f32 + a minimum per key
    auto fold = [&](const hm_v16f (&acc)[HM_CB]) {
#pragma unroll
        for (int i = 0; i < 16; i++)
#pragma unroll
            for (int cb = 0; cb < HM_CB; cb++) {
                const float kx = acc[cb][i];
                m2[cb] = hm_med3(m1[cb], m2[cb], kx); m1[cb] = hm_min(m1[cb], kx);
            }
    };
    const int ngroups = (ntiles + HM_TT - 1) / HM_TT;
    Raw nxt = fetch(0);
    if (ngroups > 0) stage(nxt, 0);
    nxt = fetch(1);
    __syncthreads();
    for (int grp = 0; grp < ngroups; grp++) {
        const int buf = grp & 1;
        if (grp + 1 < ngroups) stage(nxt, buf ^ 1);
        if (grp + 2 < ngroups) nxt = fetch(grp + 2);
        if (wave_live) {
#pragma unroll
            for (int sub = 0; sub < HM_TT; sub++) {
                const int tile = grp * HM_TT + sub;
                if (tile < ntiles) {
                    hm_v16f acc[HM_CB];
                    mma(tile, buf, sub, acc);
                    fold(acc);
                }
            }
        }
        __syncthreads();
    }
    // ---- the two lane halves saw disjoint trains of the same query: merge, add popc(query), write
#pragma unroll
    for (int cb = 0; cb < HM_CB; cb++) {
        const float o1 = __shfl_xor(m1[cb], 32, 64), o2 = __shfl_xor(m2[cb], 32, 64);
        const float b1 = min(m1[cb], o1);
        const float b2 = min(max(m1[cb], o1), min(m2[cb], o2));
        const int qi = q0 + 32 * cb + r;
        if (h == 0 && qi < nq) {
            const long long o = (long long)pair * nq + qi;
            const bool live = qi < nqp;
            const bool has1 = live && b1 < HM_SENT, has2 = live && b2 < HM_SENT;
            const int k1 = (int)b1, k2 = (int)b2;                                     // (integers below 2^24, exact)
            const int bd = has1 ? (k1 >> HM_IDX_BITS) - HM_BIAS + pa[cb] : 256;
            best_idx[o] = bd < 256 ? (k1 & ((1 << HM_IDX_BITS) - 1)) : -1;           // the reference starts at 256 and compares with <
            best_dist[o] = bd;
            second_dist[o] = has2 ? (k2 >> HM_IDX_BITS) - HM_BIAS + pa[cb] : 256;
        }
    }
}

// Known-answer tap of the FP4 tile (ccm_debug_fp4_tile): out[i][j] = 32 x 32 x 256 product of train rows a (32 x 32 bytes) and query
// rows b through hm_expand32_fp4 and the four matrix instructions exactly as k_hamming_mfma issues them, on top of c[i] in every column.
__global__ __launch_bounds__(64) void k_fp4_tile(const unsigned* __restrict__ a, const unsigned* __restrict__ b, const float* __restrict__ c,
                                                 float* __restrict__ out)
{
    const int lane = threadIdx.x, h = lane >> 5, r = lane & 31;
    hm_v16f acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = c[(i & 3) + 8 * (i >> 2) + 4 * h];
#pragma unroll
    for (int s = 0; s < 4; s++) acc = hm_mfma(hm_expand32_fp4(a[8 * r + 4 * h + s], 2u), hm_expand32_fp4(b[8 * r + 4 * h + s], 10u), acc);
#pragma unroll
    for (int i = 0; i < 16; i++) out[32 * ((i & 3) + 8 * (i >> 2) + 4 * h) + r] = acc[i];
}
void match_launch_fp4_tile(hipStream_t s, const unsigned* a, const unsigned* b, const float* c, float* out)
{
    hipLaunchKernelGGL(k_fp4_tile, dim3(1), dim3(64), 0, s, a, b, c, out);
}

// Exact merge of per-split partial results over disjoint, ascending index ranges: the overall best is the
// lexicographic minimum of (dist, index); the overall second-smallest distance is
// min(max(best_a, best_b), second_a, second_b) folded over the splits in index order.
__global__ __launch_bounds__(256) void k_hamming_merge(const unsigned* __restrict__ part_best, const int* __restrict__ part_second,
                                                       int n_pairs, int nq, int n_split, const int* __restrict__ nq_n,
                                                       int* __restrict__ best_idx, int* __restrict__ best_dist, int* __restrict__ second_dist)
{
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= (long long)n_pairs * nq) return;
    const int pair = (int)(i / nq), qi = (int)(i - (long long)pair * nq);
    const int nqp = nq_n ? min(max(nq_n[pair], 0), nq) : nq;
    unsigned best = (256u << 16) | 0xFFFFu; int sec = 256;
    for (int s = 0; s < n_split; s++) {
        const long long o = ((long long)pair * n_split + s) * nq + qi;
        const unsigned b = part_best[o]; const int sc = part_second[o];
        sec = min(min(sec, sc), max((int)(best >> 16), (int)(b >> 16)));
        best = min(best, b);
    }
    const bool live = qi < nqp;
    best_idx[i] = (live && (best >> 16) < 256u) ? (int)(best & 0xFFFFu) : -1;
    best_dist[i] = live ? (int)(best >> 16) : 256;
    second_dist[i] = live ? sec : 256;
}

// Distances of side-1 feature i to the side-2 features order2[start[i] .. start[i]+len[i]) (its vocabulary
// node, ascending feature index), written to dist[off[i] ..].  One wave per feature: lanes stride the range.
__global__ __launch_bounds__(256) void k_hamming_ranges(
    const uint8_t* __restrict__ d1, const uint8_t* __restrict__ d2, const int* __restrict__ order2,
    const int* __restrict__ start, const int* __restrict__ len, const long long* __restrict__ off, int n1,
    unsigned short* __restrict__ dist)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n1) return;
    const int L = len[i];
    if (L <= 0) return;
    const uint4* a = reinterpret_cast<const uint4*>(d1) + 2 * (long long)i;
    const uint4 a0 = a[0], a1 = a[1];
    const int s = start[i];
    unsigned short* o = dist + off[i];
    for (int k = lane; k < L; k += 64) {
        const uint4* b = reinterpret_cast<const uint4*>(d2) + 2 * (long long)order2[s + k];
        o[k] = (unsigned short)ham256(a0, a1, b[0], b[1]);
    }
}

// the matrix cores while the row words fit their LDS table, else the vector-ALU kernel (n_split workgroups per pair) plus the merge
void match_launch_bf(hipStream_t s, const uint8_t* q, long long q_pair_bytes, const uint8_t* t, long long t_pair_bytes,
                     int nq, int nt, int n_pairs, const int* nq_n, const int* nt_n, int n_split,
                     unsigned* part_best, int* part_second, int* bi, int* bd, int* sd)
{
    if (nt <= HM_MAX_NT) {
        const int q_blocks = (nq + HM_QW * HM_WAVES - 1) / (HM_QW * HM_WAVES);
        hipLaunchKernelGGL(k_hamming_mfma<>, dim3(n_pairs * q_blocks), dim3(HM_TPB), 0, s, q, q_pair_bytes, t, t_pair_bytes, nq, nt, nq_n, nt_n,
                           q_blocks, bi, bd, sd);
        return;
    }
    hipLaunchKernelGGL(k_hamming_bf, dim3(n_pairs * n_split), dim3(BF_THREADS), 0, s, q, q_pair_bytes, t, t_pair_bytes, nq, nt, nq_n, nt_n, n_split,
                       part_best, part_second, bi, bd, sd);
    if (n_split > 1)
        hipLaunchKernelGGL(k_hamming_merge, dim3((unsigned)(((long long)n_pairs * nq + 255) / 256)), dim3(256), 0, s,
                           part_best, part_second, n_pairs, nq, n_split, nq_n, bi, bd, sd);
}
void match_launch_ranges(hipStream_t s, const uint8_t* d1, const uint8_t* d2, const int* order2, const int* start,
                         const int* len, const long long* off, int n1, unsigned short* dist)
{
    hipLaunchKernelGGL(k_hamming_ranges, dim3((n1 + 3) / 4), dim3(256), 0, s, d1, d2, order2, start, len, off, n1, dist);
}
