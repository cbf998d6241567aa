// orb_pyramid.hip -- the image pyramid of the ORB extractor: one cv::resize per level (the stages: orb_types.h).
#include <hip/hip_runtime.h>
#include "orb_types.h"
#include "orb_device.h"

// ------------------------------------------------------------------------------------------------
// k_pyr_resize: one thread = 4 horizontally adjacent output pixels in each of RS_ROWS consecutive rows: the x tables
// are loaded once, and the 2 * RS_ROWS source loads are independent and issued together (the kernel is bound by
// dependent-load latency, not by bytes or ALU).
// Fixed-point bilinear exactly as cv::resize(INTER_LINEAR) for 8-bit data:
// weights are the host-made 11-bit tables, horizontal pass int32, vertical pass
// ((b0*(r0>>4))>>16) + ((b1*(r1>>4))>>16) + 2 >> 2.
// Round 3 built the streaming alternative -- a wave walks 32 output rows of its 256-column strip, loads every source row once (6 rows
// requested ahead), keeps its horizontal pass for the two output rows that need it (3.6 instead of 6 loaded dwords per output row) --
// bit-exact, and slower: 0.270 against 0.173 ms for the seven levels.  Its serial row loop needs selects, moves and address arithmetic
// that the fully unrolled kernel below does not (18 against 14 vector instructions per pixel), and a quarter of the waves.  Not kept.
// Built, measured and dropped (profiles/fe_prelude_ab.txt): the head on a flat argument block -- what the kernel uses of the two level
// records as 16 scalars and pointers instead of OrbGeom by value and a level index (g.lv[level] is a scalar load whose address depends
// on another: four dependent scalar waits stand in front of the y-table loads), the first 14 dwords preloaded, the x tables requested
// with the y tables instead of behind the v_readlane broadcasts, the status clear last.  Bit-exact, but 65 VGPRs where this kernel has
// 64 (seven waves per SIMD; held to eight it spills), and 0.1723-0.1739 against 0.1704-0.1730 ms, step 0.7800-0.7844 against
// 0.7775-0.7801 ms.  The head of this kernel has not been stamped.
#ifndef RS_ROWS
#define RS_ROWS 8                // rows per thread (measured: 4 -> 0.186, 8 -> 0.172, 16 -> 0.260 ms)
#endif
// clear_status: the extractor's status word, zeroed by the first thread of the launch that opens a call (nullptr otherwise) -- stream
// order puts that before every kernel that ORs into the word, and a fill dispatch of its own is saved.
__global__ __launch_bounds__(256) void k_pyr_resize(const OrbGeom g, int level, int* __restrict__ clear_status)
{
    if (clear_status && (blockIdx.x | blockIdx.y | blockIdx.z | threadIdx.x) == 0) *clear_status = 0;
    const OrbLevel& D = g.lv[level];
    const OrbLevel& S = g.lv[level - 1];
    const int lane = threadIdx.x & 63;
    const int x4 = (blockIdx.x * 64 + lane) * 4;
    // everything that depends on the row only is wave-uniform: kept in scalar registers
    const int yb = (blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * RS_ROWS;
    const int f = blockIdx.z + g.frame0;
    if (yb >= D.h) return;
    const uint8_t* src = S.img + (long long)f * S.plane;
    uint8_t* dstp = const_cast<uint8_t*>(D.img) + (long long)f * D.plane;
    // lanes 0..RS_ROWS-1 fetch the y tables of the wave's rows; v_readlane broadcasts them
    int yo; unsigned ybb;
    {
        const int y = min(yb + (lane & (RS_ROWS - 1)), D.h - 1);
        yo = D.yofs[y];
        __builtin_memcpy(&ybb, D.yab + 2 * y, 4);
    }
    const uint8_t* r0p[RS_ROWS]; const uint8_t* r1p[RS_ROWS]; unsigned b0[RS_ROWS], b1[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        const int sy0 = __builtin_amdgcn_readlane(yo, r);
        const unsigned bb = (unsigned)__builtin_amdgcn_readlane((int)ybb, r);
        r0p[r] = src + (long long)sy0 * S.pitch;
        r1p[r] = src + (long long)min(sy0 + 1, S.h - 1) * S.pitch;
        b0[r] = bb & 0xFFFFu; b1[r] = bb >> 16;
    }
    if (x4 >= D.w) return;
    {
        // tables of the 4 outputs: two 16-byte loads (the tables are only 4-/2-byte aligned); the last, partial quad of
        // a row repeats its last column (the bytes past D.w land in the row padding, which nothing reads as data)
        int sxs[4]; unsigned abw[4];
        if (x4 + 3 < D.w) {
            int4 so; uint4 ab;
            __builtin_memcpy(&so, D.xofs + x4, 16);
            __builtin_memcpy(&ab, D.xab + 2 * x4, 16);
            sxs[0] = so.x; sxs[1] = so.y; sxs[2] = so.z; sxs[3] = so.w;
            abw[0] = ab.x; abw[1] = ab.y; abw[2] = ab.z; abw[3] = ab.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int x = min(x4 + i, D.w - 1);
                sxs[i] = D.xofs[x];
                __builtin_memcpy(&abw[i], D.xab + 2 * x, 4);
            }
        }
        // The 4 outputs read source columns base .. base+7 at most.  At the right border the 8-byte window is pulled
        // back inside the row (the neighbour weight of the last column is 0, so its clamped byte is never used), and
        // the 12-byte fetch is pulled back inside the pitch: every lane takes this path, no divergent border code.
        const int base = min(sxs[0], S.w - 8);
        const int ba = min(base & ~3, S.pitch - 12);
        if (S.w >= 8 && S.pitch >= 12 && sxs[3] - base <= 7) {
            uint2 q0[RS_ROWS], q1[RS_ROWS];
            const unsigned sh = (unsigned)(base - ba);            // 0..4
            const bool sh4 = sh > 3u;
#pragma unroll
            for (int r = 0; r < RS_ROWS; r++) {
                const unsigned* p0 = reinterpret_cast<const unsigned*>(r0p[r] + (unsigned)ba);
                const unsigned* p1 = reinterpret_cast<const unsigned*>(r1p[r] + (unsigned)ba);
                const unsigned d00 = p0[0], d01 = p0[1], d02 = p0[2], d10 = p1[0], d11 = p1[1], d12 = p1[2];
                const unsigned l0 = sh4 ? d01 : d00, m0 = sh4 ? d02 : d01, l1 = sh4 ? d11 : d10, m1 = sh4 ? d12 : d11;
                q0[r].x = __builtin_amdgcn_alignbyte(m0, l0, sh); q0[r].y = __builtin_amdgcn_alignbyte(d02, m0, sh);   // v_alignbyte uses sh & 3
                q1[r].x = __builtin_amdgcn_alignbyte(m1, l1, sh); q1[r].y = __builtin_amdgcn_alignbyte(d12, m1, sh);
            }
            unsigned sel[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const unsigned o = (unsigned)(sxs[i] - base);
                sel[i] = 0x0c000c00u + o + (min(o + 1u, 7u) << 16);   // v_perm_b32: bytes o and o+1 as a u16 pair
            }
#pragma unroll
            for (int r = 0; r < RS_ROWS; r++) {
                unsigned out = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    // v_dot2_u32_u16 applies the packed (a0,a1) weights
                    const unsigned h0 = __builtin_amdgcn_udot2(fc_pk(__builtin_amdgcn_perm(q0[r].y, q0[r].x, sel[i])), fc_pk(abw[i]), 0u, false);
                    const unsigned h1 = __builtin_amdgcn_udot2(fc_pk(__builtin_amdgcn_perm(q1[r].y, q1[r].x, sel[i])), fc_pk(abw[i]), 0u, false);
                    // b <= 2048 and h >> 4 < 2^15: 24-bit multiplies are exact; the result is <= 255
                    const unsigned v = ((__umul24(b0[r], h0 >> 4) >> 16) + (__umul24(b1[r], h1 >> 4) >> 16) + 2u) >> 2;
                    out |= v << (8 * i);
                }
                if (yb + r < D.h) *reinterpret_cast<unsigned*>(dstp + (long long)(yb + r) * D.pitch + (unsigned)x4) = out;
            }
            return;
        }
    }
    for (int r = 0; r < RS_ROWS && yb + r < D.h; r++) {
        unsigned out = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int x = min(x4 + i, D.w - 1);
            const int sx0 = D.xofs[x];
            const int sx1 = min(sx0 + 1, S.w - 1);
            const int a0 = D.xab[2 * x], a1 = D.xab[2 * x + 1];
            const int h0 = r0p[r][sx0] * a0 + r0p[r][sx1] * a1;
            const int h1 = r1p[r][sx0] * a0 + r1p[r][sx1] * a1;
            const int v = ((((int)b0[r] * (h0 >> 4)) >> 16) + (((int)b1[r] * (h1 >> 4)) >> 16) + 2) >> 2;
            out |= (unsigned)(v & 255) << (8 * i);
        }
        // our level buffers have pitch % 64 == 0 and a 256-byte aligned base: the dword store is aligned
        *reinterpret_cast<unsigned*>(dstp + (long long)(yb + r) * D.pitch + (unsigned)x4) = out;
    }
}

void orb_launch_resize(hipStream_t s, const OrbGeom& g_dev, int level, int dw, int dh, int nframes, int* clear_status)
{
    dim3 grid((dw + 255) / 256, (dh + 4 * RS_ROWS - 1) / (4 * RS_ROWS), nframes);
    hipLaunchKernelGGL(k_pyr_resize, grid, dim3(256), 0, s, g_dev, level, clear_status);
}
