// orb_device.h -- device helpers that more than one stage of the ORB extractor uses (the stages: orb_types.h).
// Wavefront = 64 everywhere; ballots are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include "orb_types.h"

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
// gx, gy: the grid's sizes.  A kernel that wants its first load early passes them as explicit arguments at the front of its argument
// block (k_fast_cells): gridDim is a load from the hidden arguments, behind everything explicit.
__device__ __forceinline__ void xcd_work_item(int on, unsigned gx, unsigned gy, int& x, int& y)
{
    x = (int)blockIdx.x; y = (int)blockIdx.y;
    if (!on) return;
    const unsigned total = gx * gy;
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
__device__ __forceinline__ void xcd_work_item(int on, int& x, int& y) { xcd_work_item(on, gridDim.x, gridDim.y, x, y); }

// Inclusive wave prefix sum by DPP, with no LDS round trip (__shfl_up is a ds_bpermute each, six of them in a chain): the row_shr
// ladder 1, 2, 4, 8 scans every row of 16 lanes (a lane whose source lies outside its row adds 0), row_bcast:15 adds the total of
// rows 0 / 2 to rows 1 / 3, row_bcast:31 the total of rows 0-1 to rows 2-3.  Needs all 64 lanes active: a DPP read of an inactive
// lane returns nothing, so call it only under wave-uniform control (k_octree's loops over 64-entry chunks are).
__device__ __forceinline__ int wave_incl_scan(int v)
{
#define WSC_STEP(ctrl, rows) v += __builtin_amdgcn_update_dpp(0, v, ctrl, rows, 0xf, false);
    WSC_STEP(0x111, 0xf)           // row_shr:1
    WSC_STEP(0x112, 0xf)           // row_shr:2
    WSC_STEP(0x114, 0xf)           // row_shr:4
    WSC_STEP(0x118, 0xf)           // row_shr:8
    WSC_STEP(0x142, 0xa)           // row_bcast:15 into rows 1, 3
    WSC_STEP(0x143, 0xc)           // row_bcast:31 into rows 2, 3
#undef WSC_STEP
    return v;
}
// the wave's total behind wave_incl_scan: lane 63's value, by v_readlane (a scalar; all lanes active or not)
__device__ __forceinline__ int wave_last(int incl) { return __builtin_amdgcn_readlane(incl, 63); }
// Wave sum by DPP (the one-value form of wave_sum2_dpp below; the same condition: all 64 lanes active).
__device__ __forceinline__ int wave_sum(int v)
{
#define WS1_STEP(ctrl, rows) v += __builtin_amdgcn_update_dpp(0, v, ctrl, rows, 0xf, false);
    WS1_STEP(0xb1, 0xf)            // quad_perm [1,0,3,2]
    WS1_STEP(0x4e, 0xf)            // quad_perm [2,3,0,1]
    WS1_STEP(0x141, 0xf)           // row_half_mirror
    WS1_STEP(0x140, 0xf)           // row_mirror
    WS1_STEP(0x142, 0xa)           // row_bcast:15 into rows 1, 3
    WS1_STEP(0x143, 0xc)           // row_bcast:31 into rows 2, 3
#undef WS1_STEP
    return __builtin_amdgcn_readlane(v, 63);
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

// ------------------------------------------------------------------------------------------------
// The items of k_fast_cells's rejection test, and the order in which its waves take them (the kernel and, through
// ccm_debug_fc_items, the host run this very code).  An item is four pixels = one dword of the band's tile that holds a detection
// column: rows 3 .. bh - 4, dwords dw_lo .. dw_hi, numbered row-major over those n_dw = dw_hi - dw_lo + 1 dwords ONLY (before, every
// dword of the row was numbered, and the lanes outside dw_lo .. dw_hi idled through their run: 4292 runs per 752x480 frame of 8
// levels against 3791).  A run is 64 consecutive items, one per lane; run R goes to wave R % FC_WAVES, so the run counts of the
// waves differ by at most one.  A lane keeps (rr, dw) = (row - 3, dword) and advances it by FC_ITEM_STRIDE = 64 * FC_WAVES items per
// run with one add, one conditional wrap and an add with carry: the quotient and remainder of FC_ITEM_STRIDE by n_dw come with
// the band record (FcEnum, orb_types.h), no multiply or divide in the loop.
#define FC_WAVES 4
#define FC_ITEM_STRIDE (64 * FC_WAVES)
struct FcItem { int rr, dw; };         // row - 3, dword of the row
__host__ __device__ inline FcEnum fc_enum(int dw_lo, int dw_hi)
{
    FcEnum e{};
    const int n = dw_hi >= dw_lo ? dw_hi - dw_lo + 1 : 0, d = n > 0 ? n : 1;
    e.n_dw = (short)n; e.d_step = (short)(FC_ITEM_STRIDE % d); e.r_step = (short)(FC_ITEM_STRIDE / d);
    e.nd_inv = (1u << 20) / (unsigned)d + 1u;
    return e;
}
// runs of a band of bh rows (none where bh <= 6 or no dword holds a detection column)
__host__ __device__ inline int fc_item_runs(int bh, int n_dw) { return bh > 6 && n_dw > 0 ? ((bh - 6) * n_dw + 63) >> 6 : 0; }
// first item of lane l of wave w: item 64 * w + l
__host__ __device__ inline FcItem fc_item_start(int dw_lo, int n_dw, unsigned nd_inv, int w, int l)
{
    const int it = 64 * w + l;
    FcItem i;
    i.rr = (int)(((unsigned)it * nd_inv) >> 20);
    i.dw = dw_lo + it - i.rr * n_dw;
    return i;
}
// the lane's item of the wave's next run: FC_ITEM_STRIDE items on (dw_end = dw_hi + 1)
__host__ __device__ inline void fc_item_step(FcItem& i, int dw_end, int n_dw, int d_step, int r_step)
{
    const int d = i.dw + d_step;
    const bool wrap = d >= dw_end;
    i.dw = wrap ? d - n_dw : d;
    i.rr += r_step + (wrap ? 1 : 0);
}
// the item is one of the band's (a lane past the last item of the last run: no)
__host__ __device__ inline bool fc_item_valid(const FcItem& i, int bh) { return i.rr < bh - 6; }
// tile offset of the item's first pixel (< 2^15: the host keeps pitch * bh below that)
__host__ __device__ inline int fc_item_pos0(const FcItem& i, int P)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(i.rr, P) + 3 * P + 4 * i.dw;        // (rr <= 58, P <= 256: a 24-bit multiply-add, not v_mul_lo_u32)
#else
    return (3 + i.rr) * P + 4 * i.dw;
#endif
}
