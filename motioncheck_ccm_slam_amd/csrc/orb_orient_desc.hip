// orb_orient_desc.hip -- orientation and descriptor of the selected keypoints of the ORB extractor (the stages: orb_types.h).
#include <hip/hip_runtime.h>
#include "orb_types.h"
#include "orb_device.h"
#include "../../include/ccm_orb_pattern.h"
#include "../../include/ccm_sincos.h"

// ------------------------------------------------------------------------------------------------
// k_orient_desc: a wave per selected keypoint (small batches) or per OD_ITEMS keypoint slots (see the kernel).
//   IC_Angle (ORBextractor.cpp:68-95) on the un-blurred level, cv::fastAtan2;
//   GaussianBlur 7x7 sigma 2 BORDER_REFLECT_101 (:1259; integer taps {18,34,49,55,49,34,18},
//   SURVEY.md 12.6) evaluated only where the pattern reads it: the row pass on the 37 columns of the
//   43-row patch, the column pass at the 512 sample points -- the sum
//   sum_ij q_i q_j src is exact in integers, so it equals the reference's full-image separable
//   blur bit for bit and the blurred pyramid is never written to HBM;
//   computeOrbDescriptor (:100-316): bit k = I(p_2k) < I(p_2k+1) with the pattern rotated by the angle.
//
// The kernel is vector-issue bound (514 VALU wave-instructions per keypoint before, 463 now; prices of the classes:
// profiles/od_diet_valu_calibration.txt), and its instruction stream was gone through part by part, every part bit-exact, each timed
// as a library of its own against the parent on one box (profiles/od_diet_ab.txt; k_orient_desc<8> per 256-frame batch, ranges over 8
// rounds, parent 0.2371-0.2385 ms in run 1 and 0.2368-0.2384 in run 2).  KEPT:
//   C  the pattern's pairs as floats in LDS (od_build_pattern; 16 SDWA conversions per keypoint less)       0.2325-0.2341
//   D  the centre offset in one pinned base, a point's four dwords off one address (od_gather_base)         0.2332-0.2351
//   E  on top of D: round to nearest even by adding 1.5 * 2^23, addresses from the biased bits (od_rn)      0.2283-0.2303
//   C + D + E = this file: 0.2254-0.2258 ms, step 0.7589-0.7638 against 0.7702-0.7745 ms.
// BUILT, MEASURED AND TAKEN OUT (fewer instructions each, no faster):
//   A  fast_atan2_deg with one division and one polynomial for both arms (-20 instructions, all on wave-uniform values): 0.2381-0.2395
//   B  ccm_sincosf's sine and cosine chains on even / odd lanes, coefficients per lane from LDS, (a, b) in scalar registers
//      (42 -> 26 f64 instructions): 0.2408-0.2420; with C + D + E 0.2357-0.2375 against 0.2253-0.2263 without it
//   F  the row blur on unshifted dwords with ten shifted weight words (92 v_dot4 and no v_alignbyte against 74 + 30): 0.2383-0.2395; the
//      dependent v_dot4 of a column then stand back to back with wait states between them, where the shifts used to fill in
//   A + C + D + E + F: 0.2271-0.2279; all six: 0.2256-0.2267.
//   E with the column term pinned into one v_mad_i32_i24 (+ v_add_u32) instead of v_mul_i32_i24 + v_add3_u32: 0.2261-0.2280 with C + D + E
//      (no better), and 0.2372-0.2382 with all six parts (as slow as the parent).
__device__ __forceinline__ int reflect101(int i, int n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ float fast_atan2_deg(float y, float x)
{
    const float scale = (float)(180.0 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * scale;
    const float p3 = -0.3258083974640975f * scale;
    const float p5 = 0.1555786518463281f * scale;
    const float p7 = -0.04432655554792128f * scale;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + 2.2204460492503131e-16f);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + 2.2204460492503131e-16f);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

static constexpr float OD_FACTOR_PI = (float)(3.14159265358979323846 / 180.f);      // degrees to radians (:103)

// Per-wave LDS: hT[37][46] u16 (horizontally blurred, transposed: column-major, so the 7 tap rows of a
// blurred pixel are 4 consecutive dwords of its column; the 92-byte pitch = 23 dwords is odd, which spreads
// the scattered gathers of the descriptor over the banks).  The vertical pass runs at the sample points only,
// so no blurred patch is stored (it used to overlay hT); 8 workgroups (32 waves) share a CU.
#define OD_HT_PITCH 92
#define OD_WAVE_LDS (ORB_BLUR_D * OD_HT_PITCH)
#define OD_WAVE_LDS_PAD ((OD_WAVE_LDS + 15) & ~15)

__constant__ signed char c_pattern[1024];

typedef unsigned short od_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned od_dot2(unsigned a, unsigned w, unsigned acc)
{
    return __builtin_amdgcn_udot2(__builtin_bit_cast(od_us2, a), __builtin_bit_cast(od_us2, w), acc, false);
}
// The blurred pixel (18 + dx, 18 + dy) of the patch: the 7 vertical taps {18,34,49,55,49,34,18} over hT rows 18+dy .. 24+dy of
// column 18+dx (|dx|, |dy| <= 18), and the single rounding.  ctr points at column 18, dword 9.  Rows are packed two per dword,
// so the taps need the 4 aligned dwords from row 18+dy rounded down to even; on an odd row v_alignbit moves the window up by one
// halfword, so one even-row tap layout serves both.  The 4th pair's upper half (weight 0) is row 25+dy or, on odd rows, zero.
// The taps sum to 257, so a saturated neighbourhood blurs to 257: the reference's saturation to 255 is needed (min before the shift,
// which the compare then folds into a halfword select).
// od_gather requests the 4 dwords and keeps the shift, od_blur_at applies the taps once they have arrived.
#ifndef OD_BRIEF_BATCH
#define OD_BRIEF_BATCH 2         // BRIEF rounds whose gathers are in flight together (1, 2 or 4)
#endif
struct OdTaps { unsigned d[4], sh; };
typedef const __attribute__((address_space(3))) unsigned od_lu32;      // a dword of LDS by its 32-bit address
// A steered coordinate rounded to nearest even, as an integer with OD_RN_BIAS added: for |t| < 2^22 the float t + 1.5 * 2^23 has
// ulp 1 and the exponent of 1.5 * 2^23, so the IEEE add rounds t exactly as v_rndne_f32 would and the sum's bit pattern is
// 0x4B400000 + rint(t).  The bias is even and its low 24 bits are positive, so od_gather works on the biased value as it is.
#define OD_RN_BIAS 0x4B400000
__device__ __forceinline__ int od_rn(float t) { return __float_as_int(t + 12582912.f); }
// the LDS address od_gather takes for a wave whose hT starts at LDS address wl: column 18, the dword of rows 18-19, less what the
// biased coordinates add (the low 24 bits of the bias times the pitch; twice the bias for the row dword); wraps mod 2^32
__device__ __forceinline__ unsigned od_gather_base(unsigned wl)
{
    return wl + 18u * OD_HT_PITCH + 4u * 9u - (unsigned)(OD_RN_BIAS & 0xFFFFFF) * OD_HT_PITCH - ((unsigned)OD_RN_BIAS << 1);
}
// dx, dy: od_rn's.  The point's four dwords are two ds_read2_b32 off one address.
__device__ __forceinline__ void od_gather(unsigned base, int dx, int dy, OdTaps& t)
{
    // column: a 24-bit multiply (the low 24 bits of dx); row: 4 * (dy >> 1) = (dy << 1) & ~3, bias included (it is even)
    const unsigned addr = (unsigned)(__mul24(dx, OD_HT_PITCH) + (int)base) + (((unsigned)dy << 1) & ~3u);
    od_lu32* p = (od_lu32*)(uintptr_t)addr;
#pragma unroll
    for (int i = 0; i < 4; i++) t.d[i] = p[i];
    t.sh = (unsigned)dy << 4;                                       // v_alignbit / v_lshrrev read bits 4:0 = 16 * (dy & 1)
}
__device__ __forceinline__ unsigned od_blur_at(const OdTaps& t)
{
    const unsigned e0 = __builtin_amdgcn_alignbit(t.d[1], t.d[0], t.sh), e1 = __builtin_amdgcn_alignbit(t.d[2], t.d[1], t.sh);
    const unsigned e2 = __builtin_amdgcn_alignbit(t.d[3], t.d[2], t.sh), e3 = t.d[3] >> (t.sh & 31u);
    const unsigned v = od_dot2(e3, 18u, od_dot2(e2, 49u | (34u << 16), od_dot2(e1, 49u | (55u << 16), od_dot2(e0, 18u | (34u << 16), 32768u))));
    return min(v, 0xFFFFFFu) >> 16;                                 // = min(v >> 16, 255)
}

// The pattern's 256 test pairs (x0, y0, x1, y1) in LDS, as floats: lane L evaluates pairs L, 64 + L, 128 + L, 192 + L of every keypoint
// of its wave, so the bytes are converted once per workgroup, not once per keypoint, and a round's pair is one ds_read_b128.
typedef float4 OdPat;
struct OdPair { float x0, y0, x1, y1; };
__device__ __forceinline__ void od_build_pattern(OdPat* pat, int tid, int nthreads)
{
    for (int i = tid; i < 256; i += nthreads) {
        const unsigned pr = *reinterpret_cast<const unsigned*>(c_pattern + 4 * i);
        pat[i] = make_float4((float)(signed char)(pr & 255u), (float)(signed char)((pr >> 8) & 255u),
                             (float)(signed char)((pr >> 16) & 255u), (float)(signed char)(pr >> 24));
    }
}
__device__ __forceinline__ OdPair od_pair(const OdPat* pat, int i)
{
    const float4 q = pat[i];
    return OdPair{ q.x, q.y, q.z, q.w };
}
// A pair's two sample points steered by (a, b) = (cos, sin) of the keypoint's angle (computeOrbDescriptor's GET_VALUE, :107-110) and
// rounded: od_rn's biased integers.
struct OdPts { int x0, y0, x1, y1; };
__device__ __forceinline__ OdPts od_steer(const OdPair& q, float a, float b)
{
    return OdPts{ od_rn(q.x0 * a - q.y0 * b), od_rn(q.x0 * b + q.y0 * a), od_rn(q.x1 * a - q.y1 * b), od_rn(q.x1 * b + q.y1 * a) };
}

#ifndef OD_WAVES
#define OD_WAVES 4               // waves per workgroup
#endif
#ifndef OD_ITEMS
#define OD_ITEMS 8               // keypoint slots per wave (2 / 4 / 8 measured: step 1.070 / 1.061 / 1.049 ms, from 1.125 with one)
#endif
// A wave works through OD_ITEMS slots.  Until round 3 it took one and ended: every keypoint then paid the workgroup launch, the
// weight tables, and the chain slot -> key -> level record -> 11 row loads before its first useful instruction, ~3,500 cycles of a
// lifetime of 23,000 in which the wave held one of the CU's 32 wave slots (profiles/r03_occupancy_sweep.txt: the kernel issues for
// 0.56 of its time at full occupancy).  Now the slots of a wave are decoded together (one lane per slot), and the patch rows of the
// NEXT keypoint are requested as soon as the horizontal blur has consumed the current ones -- into the same registers -- so they
// arrive under the vertical blur and the descriptor.
struct OdItem { const uint8_t* img; int pitch, w, h, cx, cy; };
__device__ __forceinline__ void od_load_patch(const OdItem& it, int lane, unsigned (&prow)[11])
{
    const int gy = reflect101(it.cy + min(lane, ORB_PATCH_D - 1) - ORB_PATCH_R, it.h);
    const uint8_t* rp = it.img + (long long)gy * it.pitch;
    if (it.cx - ORB_PATCH_R >= 0 && it.cx + ORB_PATCH_R + 1 < it.w) {     // wave-uniform: patch inside the row
        const uint8_t* p0 = rp + it.cx - ORB_PATCH_R;
#pragma unroll
        for (int i = 0; i < 11; i++) __builtin_memcpy(&prow[i], p0 + 4 * i, 4);   // unaligned dword loads
    } else {                                                               // BORDER_REFLECT_101 columns
#pragma unroll
        for (int i = 0; i < 11; i++) {
            unsigned v = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) v |= (unsigned)rp[reflect101(it.cx + 4 * i + j - ORB_PATCH_R, it.w)] << (8 * j);
            prow[i] = v;
        }
    }
}
template <int ITEMS>
__global__ __launch_bounds__(64 * OD_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_orient_desc(const OrbGeom g, const unsigned* __restrict__ sel,
                                                     const int* __restrict__ sel_count,
                                                     ccm_keypoint* __restrict__ kps, uint8_t* __restrict__ desc,
                                                     int* __restrict__ counts, int max_per_image, int* __restrict__ status, int xcd_on)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[OD_WAVES][OD_WAVE_LDS_PAD];
    // IC_Angle weights per |v| and patch dword k (columns 4k..4k+3, u = column - 21):
    //   wone = 1 inside the disc row, wu = u + 16 inside (so that sum u*I = dot(wu) - 16*dot(wone) stays unsigned)
    __shared__ unsigned wone[16][11], wu[16][11];
    __shared__ __attribute__((aligned(16))) OdPat pat[256];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id();
    int wx, wy;
    xcd_work_item(xcd_on, wx, wy);
    const int f = wy + g.frame0;
    // ---- this wave's slots, one per lane: slot -> (level, k); output row = keypoints of lower levels + k (level-major order, :1249-1276)
    const int* sc = sel_count + (long long)f * g.nlevels;
    const int slot = (wx * ITEMS + min(lane, ITEMS - 1)) * OD_WAVES + wv;
    const unsigned key_l = slot < g.out_per_frame ? sel[(long long)f * g.out_per_frame + slot] : 0u;     // (requested before the tables are built)
    // the 256 test pairs (x0, y0, x1, y1 as signed bytes): read from LDS per keypoint (as global loads they put a wait for ALL of the
    // wave's outstanding memory operations, the previous descriptor stores included, in front of each of the four rounds)
    od_build_pattern(pat, threadIdx.x, 64 * OD_WAVES);
    for (int i = threadIdx.x; i < 16 * 11; i += 64 * OD_WAVES) {
        const int av = i / 11, k = i - av * 11;
        const int lim = g.umax[av];
        unsigned a = 0, b = 0;
        for (int j = 0; j < 4; j++) {
            const int u = 4 * k + j - ORB_PATCH_R;
            if (u >= -lim && u <= lim) { a |= 1u << (8 * j); b |= (unsigned)(u + 16) << (8 * j); }
        }
        wone[av][k] = a; wu[av][k] = b;
    }
    int level_l = 0, first_l = 0;
    for (int l = 1; l < g.nlevels; l++) if (slot >= g.lv[l].out_first) { level_l = l; first_l = g.lv[l].out_first; }
    int row_l = slot - first_l, tot = 0, cnt_l = 0;
    for (int l = 0; l < g.nlevels; l++) { const int c = sc[l]; if (l < level_l) row_l += c; if (l == level_l) cnt_l = c; tot += c; }
    if (wx == 0 && wv == 0 && lane == 0) {
        counts[f] = min(tot, max_per_image);
        if (tot > max_per_image) atomicOr(status, 8);
    }
    if (wx == 0) {                                                         // the frame's rows past its count are zero, not left from an earlier call
        const long long r0 = (long long)f * max_per_image + min(tot, max_per_image);
        const int npad = max_per_image - min(tot, max_per_image);
        unsigned* kz = reinterpret_cast<unsigned*>(kps + r0);             // (7 dwords per keypoint row)
        for (int i = threadIdx.x; i < npad * 7; i += 64 * OD_WAVES) kz[i] = 0u;
        uint4* dz = reinterpret_cast<uint4*>(desc + r0 * 32);
        for (int i = threadIdx.x; i < npad * 2; i += 64 * OD_WAVES) dz[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    const bool valid_l = lane < ITEMS && slot < g.out_per_frame && slot - first_l < cnt_l && row_l < max_per_image;
    unsigned long long todo = __ballot(valid_l);
    __syncthreads();                                                       // (the weight tables)
    if (todo == 0) return;

    uint8_t* wl = lds[wv];
    auto item_of = [&](int j, OdItem& it, int& level, int& score, int& row) {
        const unsigned key = (unsigned)__builtin_amdgcn_readlane((int)key_l, j);
        level = __builtin_amdgcn_readlane(level_l, j); row = __builtin_amdgcn_readlane(row_l, j);
        const OrbLevel& L = g.lv[level];
        it.img = L.img + (long long)f * L.plane; it.pitch = L.pitch; it.w = L.w; it.h = L.h;
        it.cx = (int)(key & 0xFFFu) + ORB_BORDER; it.cy = (int)((key >> 12) & 0xFFFu) + ORB_BORDER;   // :1012-1013
        score = (int)(key >> 24);
    };
    // ---- lane r < 43 holds patch row r (43 pixels + 1 spare byte) in 11 registers
    unsigned prow[11];
    OdItem it; int level, score, row;
    {
        const int j = __builtin_ctzll(todo); todo &= todo - 1;
        item_of(j, it, level, score, row);
        od_load_patch(it, lane, prow);
    }
    for (;;) {
        // ---- IC_Angle: integer moments over the radius-15 disc, one row per lane
        int m10 = 0, m01 = 0;
        {
            const int v = lane - ORB_PATCH_R, av = v < 0 ? -v : v;
            if (av <= ORB_HALF_PATCH) {
                unsigned s1 = 0, su = 0;
#pragma unroll
                for (int i = 1; i < 10; i++) {          // columns 4..39 cover u = -15..15 (columns 6..36)
                    s1 = __builtin_amdgcn_udot4(prow[i], wone[av][i], s1, false);
                    su = __builtin_amdgcn_udot4(prow[i], wu[av][i], su, false);
                }
                m10 = (int)su - 16 * (int)s1;
                m01 = v * (int)s1;
            }
        }
        wave_sum2_dpp(m10, m01);
        const float angle = fast_atan2_deg((float)m01, (float)m10);

        // ---- horizontal 7 taps {18,34,49,55,49,34,18}: two v_dot4_u32_u8 per output, written transposed.  The previous
        //      keypoint's gathers from hT completed before its ballots; the wait keeps it so whatever the compiler schedules.
        __builtin_amdgcn_s_waitcnt(0xc07f);
        if (lane < ORB_PATCH_D) {
            const unsigned Q0 = 18u | (34u << 8) | (49u << 16) | (55u << 24), Q1 = 49u | (34u << 8) | (18u << 16);
#pragma unroll
            for (int x = 0; x < ORB_BLUR_D; x++) {
                const int kk = x >> 2, sh = x & 3;
                const unsigned w0 = sh ? __builtin_amdgcn_alignbyte(prow[kk + 1], prow[kk], sh) : prow[kk];
                const unsigned w1 = sh ? __builtin_amdgcn_alignbyte(prow[kk + 2 > 10 ? 10 : kk + 2], prow[kk + 1], sh) : prow[kk + 1];
                const unsigned h = __builtin_amdgcn_udot4(w1, Q1, __builtin_amdgcn_udot4(w0, Q0, 0u, false), false);   // <= 65535
                *reinterpret_cast<unsigned short*>(wl + x * OD_HT_PITCH + 2 * lane) = (unsigned short)h;
            }
        }
        // ---- the next keypoint's rows, into the registers the horizontal pass has just finished with
        const bool more = todo != 0;
        const int cx = it.cx, cy = it.cy, level_c = level, score_c = score, row_c = row;
        if (more) {
            const int j = __builtin_ctzll(todo); todo &= todo - 1;
            item_of(j, it, level, score, row);
            od_load_patch(it, lane, prow);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();

        // ---- steered BRIEF: lane L evaluates pairs L, 64+L, 128+L, 192+L; a ballot is 8 descriptor bytes.  The vertical taps are
        //      applied at the 512 sample points only (od_blur_at), straight from hT: no blurred patch is built.
        float a, b;
        ccm_sincosf(angle * OD_FACTOR_PI, &b, &a);
        uint8_t* drow = desc + ((long long)f * max_per_image + row_c) * 32;
        // one uniform value that the compiler cannot take apart again: left alone it adds the centre offset (too large for ds_read2_b32's
        // 8-bit offsets) to every point's address
        unsigned ctr = od_gather_base((unsigned)(uintptr_t)(const __attribute__((address_space(3))) uint8_t*)wl);
        asm volatile("" : "+s"(ctr));
        unsigned long long mybits = 0;
        // OD_BRIEF_BATCH rounds' gathers are requested before the first of them is used (the scheduler, left alone, waits for each
        // point's two reads before it requests the next point's)
#pragma unroll
        for (int r0 = 0; r0 < 4; r0 += OD_BRIEF_BATCH) {
            OdTaps tp[OD_BRIEF_BATCH][2];
#pragma unroll
            for (int q = 0; q < OD_BRIEF_BATCH; q++) {
                const OdPts pt = od_steer(od_pair(pat, (r0 + q) * 64 + lane), a, b);
                od_gather(ctr, pt.x0, pt.y0, tp[q][0]);
                od_gather(ctr, pt.x1, pt.y1, tp[q][1]);
            }
            if (OD_BRIEF_BATCH > 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < OD_BRIEF_BATCH; q++) {
                const unsigned long long bits = __ballot(od_blur_at(tp[q][0]) < od_blur_at(tp[q][1]));
                if (lane == r0 + q) mybits = bits;
            }
        }
        if (lane < 4) *reinterpret_cast<unsigned long long*>(drow + 8 * lane) = mybits;      // one 32-byte store
        if (lane == 0) {
            const OrbLevel& L = g.lv[level_c];
            ccm_keypoint kp;
            kp.x = (float)cx; kp.y = (float)cy;
            if (level_c != 0) { kp.x *= L.scale; kp.y *= L.scale; }              // :1268-1274
            kp.size = L.kp_size; kp.angle = angle; kp.response = (float)score_c;
            kp.octave = level_c; kp.class_id = -1;
            kps[(long long)f * max_per_image + row_c] = kp;
        }
        if (!more) break;
        // (the BRIEF gathers from hT are in registers -- the ballots consumed them -- before the next horizontal pass overwrites it)
    }
}

// ccm_debug_od_steer's kernel: a wave per moment pair, through the device functions k_orient_desc calls for the angle, for (a, b) and
// for the steered, rounded sample points (lane L: pairs L, 64 + L, 128 + L, 192 + L, as there).
__global__ __launch_bounds__(64) void k_od_steer_debug(const int* __restrict__ m01, const int* __restrict__ m10, int n,
                                                       float* __restrict__ angle_deg, float* __restrict__ ab, signed char* __restrict__ offs)
{
    __shared__ __attribute__((aligned(16))) OdPat pat[256];
    od_build_pattern(pat, threadIdx.x, 64);
    __syncthreads();
    const int i = blockIdx.x, lane = lane_id();
    if (i >= n) return;
    const float angle = fast_atan2_deg((float)m01[i], (float)m10[i]);
    float a, b;
    ccm_sincosf(angle * OD_FACTOR_PI, &b, &a);
    if (lane == 0) { angle_deg[i] = angle; ab[2 * i] = a; ab[2 * i + 1] = b; }
    for (int r = 0; r < 4; r++) {
        const int pair = r * 64 + lane;
        const OdPts pt = od_steer(od_pair(pat, pair), a, b);
        const int v[4] = { pt.x0 - OD_RN_BIAS, pt.y0 - OD_RN_BIAS, pt.x1 - OD_RN_BIAS, pt.y1 - OD_RN_BIAS };
        signed char* o = offs + ((long long)i * 512 + 2 * pair) * 2;
        for (int j = 0; j < 4; j++) o[j] = (signed char)min(max(v[j], -128), 127);
    }
}

extern "C" hipError_t orb_upload_pattern()
{
    return hipMemcpyToSymbol(HIP_SYMBOL(c_pattern), ccm_orb_pattern, 1024);
}
void orb_launch_od_steer_debug(hipStream_t s, const int* m01, const int* m10, int n, float* angle_deg, float* ab, int8_t* offs)
{
    hipLaunchKernelGGL(k_od_steer_debug, dim3(n), dim3(64), 0, s, m01, m10, n, angle_deg, ab, reinterpret_cast<signed char*>(offs));
}
void orb_launch_orient_desc(hipStream_t s, const OrbGeom& g_dev, int out_per_frame, int nframes, const unsigned* sel,
                            const int* sel_count, ccm_keypoint* kps, uint8_t* desc, int* counts, int max_per_image,
                            int* status)
{
    static const int xcd_on = getenv("CCM_ORB_XCD") ? atoi(getenv("CCM_ORB_XCD")) : 1;
    // a wave per slot while that still fills the GPU only a few times over (a single frame is 1,032 waves: eight slots per wave would be
    // 33 workgroups working through their slots one after the other), OD_ITEMS slots per wave for batches
    if ((long long)out_per_frame * nframes < 4 * 8192)
        hipLaunchKernelGGL(k_orient_desc<1>, dim3((out_per_frame + OD_WAVES - 1) / OD_WAVES, nframes), dim3(64 * OD_WAVES), 0, s,
                           g_dev, sel, sel_count, kps, desc, counts, max_per_image, status, xcd_on);
    else
        hipLaunchKernelGGL(k_orient_desc<OD_ITEMS>, dim3((out_per_frame + OD_WAVES * OD_ITEMS - 1) / (OD_WAVES * OD_ITEMS), nframes), dim3(64 * OD_WAVES), 0, s,
                           g_dev, sel, sel_count, kps, desc, counts, max_per_image, status, xcd_on);
}
