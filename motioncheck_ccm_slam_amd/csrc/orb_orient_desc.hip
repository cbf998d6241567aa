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
__device__ __forceinline__ void od_gather(const uint8_t* ctr, int dx, int dy, OdTaps& t)
{
    const unsigned* p = reinterpret_cast<const unsigned*>(ctr + __mul24(dx, OD_HT_PITCH) + 4 * (dy >> 1));
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
    __shared__ unsigned wone[16][11], wu[16][11], pat[256];
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
    for (int i = threadIdx.x; i < 256; i += 64 * OD_WAVES) pat[i] = *reinterpret_cast<const unsigned*>(c_pattern + 4 * i);
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
    const float factorPI = (float)(3.14159265358979323846 / 180.f);
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
        ccm_sincosf(angle * factorPI, &b, &a);
        uint8_t* drow = desc + ((long long)f * max_per_image + row_c) * 32;
        const uint8_t* ctr = wl + 18 * OD_HT_PITCH + 4 * 9;          // column 18, the dword of rows 18-19 (blurred row 18's first tap)
        unsigned long long mybits = 0;
        // OD_BRIEF_BATCH rounds' gathers are requested before the first of them is used (the scheduler, left alone, waits for each
        // point's two reads before it requests the next point's)
#pragma unroll
        for (int r0 = 0; r0 < 4; r0 += OD_BRIEF_BATCH) {
            OdTaps tp[OD_BRIEF_BATCH][2];
#pragma unroll
            for (int q = 0; q < OD_BRIEF_BATCH; q++) {
                const unsigned pr = pat[(r0 + q) * 64 + lane];
                const float x0 = (float)(signed char)(pr & 255u), y0 = (float)(signed char)((pr >> 8) & 255u);
                const float x1 = (float)(signed char)((pr >> 16) & 255u), y1 = (float)(signed char)(pr >> 24);
                od_gather(ctr, __float2int_rn(x0 * a - y0 * b), __float2int_rn(x0 * b + y0 * a), tp[q][0]);
                od_gather(ctr, __float2int_rn(x1 * a - y1 * b), __float2int_rn(x1 * b + y1 * a), tp[q][1]);
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

extern "C" hipError_t orb_upload_pattern()
{
    return hipMemcpyToSymbol(HIP_SYMBOL(c_pattern), ccm_orb_pattern, 1024);
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
