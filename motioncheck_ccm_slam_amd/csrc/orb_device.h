// orb_device.h -- device helpers that more than one stage of the ORB extractor uses (the stages: orb_types.h).
// Wavefront = 64 everywhere; ballots are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

#define WAVE 64

// a dword as two u16 lanes of the packed VALU / v_dot2_u32_u16 (k_pyr_resize's weights, k_fast_cells's rejection test)
typedef unsigned short fc_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ fc_us2 fc_pk(unsigned x) { return __builtin_bit_cast(fc_us2, x); }

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ unsigned long long lanemask_lt() { return (1ull << lane_id()) - 1ull; }

// XCD-aware work order for 2-D grids (x = item of a frame, y = frame).  Workgroups are dealt to the 8 XCDs round-robin by their
// linear id, and each XCD has its own 4 MiB L2: with the natural order the bands / keypoints of ONE frame are spread over all
// eight, so every 128-byte line of the frame's pyramid that two neighbouring items share crosses the fabric once per XCD (the
// round-1 counters showed 2.1x the algorithmic bytes for k_fast_cells).  This bijection hands XCD k a CONTIGUOUS range of
// (frame, item) pairs instead -- whole frames -- so a line is fetched once and then found in that XCD's L2.  Speed only: the
// result does not depend on where a workgroup runs.  on == 0 keeps the natural order, 1 = one contiguous range per XCD,
// C > 1 = chunks of C consecutive items per XCD, dealt cyclically (CCM_ORB_XCD, for A/B timing).
__device__ __forceinline__ void xcd_work_item(int on, int& x, int& y)
{
    x = (int)blockIdx.x; y = (int)blockIdx.y;
    if (!on) return;
    const unsigned gx = gridDim.x, total = gx * gridDim.y;
    const unsigned lin = blockIdx.y * gx + blockIdx.x;
    unsigned w;
    if (on == 1) {                                                         // each XCD one contiguous eighth of the items
        const unsigned xcd = lin & 7u, q = total >> 3, rem = total & 7u;
        w = xcd * q + (xcd < rem ? xcd : rem) + (lin >> 3);                // start of the XCD's range + its (lin / 8)-th slot
    } else {                                                               // chunk-cyclic: chunks of `on` consecutive items go to one XCD, chunk c to XCD c % 8
        const unsigned C = (unsigned)on, span = 8u * C;
        const unsigned full = total - total % span;                        // the ragged tail keeps the natural order
        if (lin >= full) w = lin;
        else {
            const unsigned xcd = lin & 7u, j = lin >> 3;                   // the XCD's j-th workgroup overall
            const unsigned super = j / C, within = j - super * C;         // j-th = `within` of the XCD's chunk number `super`
            w = (super * 8u + xcd) * C + within;
        }
    }
    // w / gx without the ~40-instruction integer division in front of every workgroup's first load (w < 2^24: exact in float)
    unsigned q = (unsigned)((float)w * __frcp_rn((float)gx));
    if (q * gx > w) q--; else if ((q + 1u) * gx <= w) q++;
    y = (int)q; x = (int)(w - q * gx);
}

// inclusive wave prefix sum
__device__ __forceinline__ int wave_incl_scan(int v)
{
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int y = __shfl_up(v, d, 64);
        if (lane >= d) v += y;
    }
    return v;
}
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// Wave sums of two ints by DPP, with no LDS round trip (wave_sum's __shfl_xor is a ds_bpermute each): quad_perm swaps, the two
// row mirrors give every lane its row's sum, row_bcast:15 / :31 carry rows 0-2 into lane 63, which is read.  The two chains
// are interleaved, so each fills the other's wait states.  Needs all 64 lanes active.  Integer sums: any order, same result.
__device__ __forceinline__ void wave_sum2_dpp(int& x, int& y)
{
#define WS2_STEP(ctrl, rows) { const int tx = __builtin_amdgcn_update_dpp(0, x, ctrl, rows, 0xf, false); \
                               const int ty = __builtin_amdgcn_update_dpp(0, y, ctrl, rows, 0xf, false); x += tx; y += ty; }
    WS2_STEP(0xb1, 0xf)            // quad_perm [1,0,3,2]
    WS2_STEP(0x4e, 0xf)            // quad_perm [2,3,0,1]
    WS2_STEP(0x141, 0xf)           // row_half_mirror
    WS2_STEP(0x140, 0xf)           // row_mirror
    WS2_STEP(0x142, 0xa)           // row_bcast:15 into rows 1, 3
    WS2_STEP(0x143, 0xc)           // row_bcast:31 into rows 2, 3
#undef WS2_STEP
    x = __builtin_amdgcn_readlane(x, 63);
    y = __builtin_amdgcn_readlane(y, 63);
}

// ------------------------------------------------------------------------------------------------
// FAST-9/16 score (k_fast_score and k_fast_cells): the largest threshold t for which the pixel is still a corner,
// i.e. max over the 16 arcs of 9 contiguous ring pixels of min(v - ring) (ring darker) or of
// min(ring - v) (ring brighter), minus one.  A pixel is a corner at threshold T iff score >= T, so
// one score map serves iniThFAST and the minThFAST fallback.  Equivalent to cv::FAST's
// cornerScore<16> for every detected corner (checked against the oracle's literal restatement).
__host__ __device__ inline int fast_score16(int v, const int* r)
{
    int d[16];
#pragma unroll
    for (int k = 0; k < 16; k++) d[k] = v - r[k];
    int lo3[16], hi3[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int a = d[k], b = d[(k + 1) & 15], c = d[(k + 2) & 15];
        lo3[k] = min(a, min(b, c));
        hi3[k] = max(a, max(b, c));
    }
    int A = -256, B = 256;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        A = max(A, min(lo3[k], min(lo3[(k + 3) & 15], lo3[(k + 6) & 15])));
        B = min(B, max(hi3[k], max(hi3[(k + 3) & 15], hi3[(k + 6) & 15])));
    }
    return max(A, -B) - 1;
}

// One polarity of that score on three-operand min/max: e[k] = ring[k] - v (brighter) or v - ring[k] (darker),
// fast_arc16(e) = max over the 16 arcs of min(e[k .. k+8]), and fast_score16(v, r) == max(arc(r - v), arc(v - r)) - 1.
// 16 + 16 + 8 instructions: w3[k] = min of 3 neighbours, w9[k] = min of three w3 = min of 9, a max3 fold over the sixteen w9.
// On the device every step is one v_min3_i32 / v_max3_i32 by name: written with min() / max() the compiler shares pairs between
// neighbouring arcs and falls back to two-operand forms (110 instructions for both polarities where 80 do).
__host__ __device__ inline int fast_min3(int a, int b, int c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int r; asm("v_min3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
#else
    return std::min(a, std::min(b, c));
#endif
}
__host__ __device__ inline int fast_max3(int a, int b, int c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int r; asm("v_max3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
#else
    return std::max(a, std::max(b, c));
#endif
}
__host__ __device__ inline int fast_mad24(int a, int b, int c)                  // a * b + c, |a|, |b| < 2^23
{
#if defined(__HIP_DEVICE_COMPILE__)
    int r; asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
#else
    return a * b + c;
#endif
}
__host__ __device__ inline int fast_arc16(const int* e)
{
    int w3[16], w9[16];
#pragma unroll
    for (int k = 0; k < 16; k++) w3[k] = fast_min3(e[k], e[(k + 1) & 15], e[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; k++) w9[k] = fast_min3(w3[k], w3[(k + 3) & 15], w3[(k + 6) & 15]);
    int m = fast_max3(w9[0], w9[1], w9[2]);
#pragma unroll
    for (int k = 3; k < 15; k += 2) m = fast_max3(m, w9[k], w9[k + 1]);
    return max(m, w9[15]);
}

// What k_fast_cells stores for a pixel that passed its rejection test -- the score where `score >= t_lo && score > 0`, else
// nothing -- from ONE polarity per pass, chosen by the four compass pixels r[0], r[4], r[8], r[12] (t_lo >= 0).
//   can_b = min(max(r0, r8), max(r4, r12)) > v + t_lo,   can_d = max(min(r0, r8), min(r4, r12)) < v - t_lo.
// Lemma.  Every arc of 9 contiguous ring pixels holds pixel 0 or 8 and pixel 4 or 12 (two pixels 8 apart cannot both be
// missed by 9 of 16), so min over the arc of (r - v) <= min(max(r0, r8), max(r4, r12)) - v.  With can_b false that is <= t_lo
// for every arc: arc(r - v) <= t_lo, the brighter polarity alone scores arc - 1 < t_lo.  Then either the full score is
// below t_lo too (nothing stored either way), or the darker polarity is >= t_lo, is the maximum, and is the full score.
// So a polarity whose flag is false never changes what `score >= t_lo && score > 0` stores.  Mirrored for can_d.
// Both flags: the polarities are scored one after the other (the kernel: in two passes).  At most one of them can store,
// since a stored score > 0 needs 9 ring pixels strictly brighter than v, or 9 strictly darker, and the ring has 16.
// `darker`: false = choose by the flags (the brighter polarity first where both hold), true = the darker polarity only (the
// second pass of a pixel with both flags).  Returns the arc value of the polarity scored; the caller stores arc - 1 where
// arc > max(t_lo, 1), which is `score >= t_lo && score > 0`.  Where NEITHER flag holds the darker polarity is scored and the
// lemma itself keeps it from storing (arc <= t_lo): no select for that case.  *again: both flags hold, the darker polarity
// is still to be scored.
__host__ __device__ inline int fast_arc16_split(int v, const int* r, int t_lo, bool darker, bool* again)
{
    const int bm = min(max(r[0], r[8]), max(r[4], r[12])), dm = max(min(r[0], r[8]), min(r[4], r[12]));
    const bool can_b = !darker && bm > v + t_lo, can_d = darker || dm < v - t_lo;
    *again = can_b && can_d;
    const int s = can_b ? 1 : -1, c = can_b ? -v : v;
    int e[16];
#pragma unroll
    for (int k = 0; k < 16; k++) e[k] = fast_mad24(s, r[k], c);         // r - v or v - r per lane: one instruction per ring pixel
    return fast_arc16(e);
}
