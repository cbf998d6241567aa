// orb_fast_tiles.hip -- FAST in two kernels through a score map in HBM: k_fast_score on 64x64 tiles, then k_cell_nms, a wave per cell.
// The path of bands that k_fast_cells (orb_fast_cells.hip) cannot hold in LDS -- LDS pitch > 256 or more than 60 KiB -- and of
// CCM_ORB_FUSED=0; both paths give the same candidates (the stages: orb_types.h).
#include <hip/hip_runtime.h>
#include "orb_types.h"
#include "orb_device.h"

// ------------------------------------------------------------------------------------------------
// k_fast_score: the FAST-9/16 score (fast_score16, orb_device.h) of every pixel of a tile, 0 where it is no corner at min(ini, min).
#define ST_W 64
#define ST_H 64            // tile height: ST_H/16 pixel rows per thread
#define ST_LW 72           // 64 + 2*4 (3-px halo rounded up to a dword on each side)
#define ST_LH (ST_H + 6)

// Phase 1: every thread applies the cheap rejection test to its pixels (4 adjacent pixels in each of
// ST_H/16 rows) and appends survivors to an LDS list (wave ballot + one LDS atomic per wave).  Phase 2:
// the list is processed densely, one survivor per lane, so the 100-instruction score never runs on a
// mostly idle wave.  Phase 3: the score tile is written as dwords.
__global__ __launch_bounds__(256) void k_fast_score(const OrbGeom g)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[ST_LH][ST_LW];
    __shared__ __attribute__((aligned(16))) uint8_t outt[ST_H][ST_W];
    __shared__ unsigned short surv[ST_W * ST_H];
    __shared__ int nsurv;
    // flattened tile index -> level
    int t = blockIdx.x, level = 0;
    for (int l = 1; l < g.nlevels; l++)
        if (t >= g.lv[l].tile_first) level = l;
    const OrbLevel& L = g.lv[level];
    t -= L.tile_first;
    const int tx0 = (t % L.tiles_x) * ST_W, ty0 = (t / L.tiles_x) * ST_H;
    const int f = blockIdx.y + g.frame0;
    const uint8_t* img = L.img + (long long)f * L.plane;
    if (threadIdx.x == 0) nsurv = 0;
    for (int i = threadIdx.x; i < ST_H * ST_W / 4; i += 256) reinterpret_cast<unsigned*>(&outt[0][0])[i] = 0u;
    // stage (clamped) pixels; clamped duplicates are only read by pixels whose score is not needed
    const bool dword_ok = ((reinterpret_cast<uintptr_t>(img) | (uintptr_t)L.pitch) & 3) == 0 && L.pitch >= ((L.w + 3) & ~3);
    if (dword_ok) {
        const int wmax = ((L.w - 1) & ~3);
        for (int i = threadIdx.x; i < ST_LH * (ST_LW / 4); i += 256) {
            const int ly = i / (ST_LW / 4), lx = i - ly * (ST_LW / 4);
            const int gy = min(max(ty0 + ly - 3, 0), L.h - 1);
            const int gx = min(max(tx0 + 4 * lx - 4, 0), wmax);
            reinterpret_cast<unsigned*>(&tile[ly][0])[lx] = *reinterpret_cast<const unsigned*>(img + (long long)gy * L.pitch + gx);
        }
    } else {
        for (int i = threadIdx.x; i < ST_LH * ST_LW; i += 256) {
            const int ly = i / ST_LW, lx = i - ly * ST_LW;
            const int gy = min(max(ty0 + ly - 3, 0), L.h - 1);
            const int gx = min(max(tx0 + lx - 4, 0), L.w - 1);
            tile[ly][lx] = img[(long long)gy * L.pitch + gx];
        }
    }
    __syncthreads();
    const int px = (threadIdx.x & 15) * 4;
    const int t_lo = min(g.ini_th, g.min_th);
    for (int py = threadIdx.x >> 4; py < ST_H; py += 16) {
        const int gy = ty0 + py;
        const bool row_ok = gy >= ORB_EDGE && gy < L.h - ORB_EDGE;
        const int cy = py + 3;
        // the 12 bytes around the 4 centre pixels and the 4 bytes three rows below / above, as dwords
        const unsigned* crow = reinterpret_cast<const unsigned*>(&tile[cy][0]) + (px >> 2);
        const unsigned c0 = crow[0], c1 = crow[1], c2 = crow[2];
        const unsigned nn = reinterpret_cast<const unsigned*>(&tile[cy + 3][0])[(px >> 2) + 1];
        const unsigned ss = reinterpret_cast<const unsigned*>(&tile[cy - 3][0])[(px >> 2) + 1];
        const unsigned long long lo = ((unsigned long long)c1 << 32) | c0, hi = ((unsigned long long)c2 << 32) | c1;
        unsigned keep4 = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int gx = tx0 + px + i;
            if (row_ok && gx >= ORB_EDGE && gx < L.w - ORB_EDGE) {
                const int v = (int)((c1 >> (8 * i)) & 0xFF);
                const int n = (int)((nn >> (8 * i)) & 0xFF), s = (int)((ss >> (8 * i)) & 0xFF);
                const int w = (int)((lo >> (8 * (i + 1))) & 0xFF);         // column cx-3 = byte 4+i-3 of the 12
                const int e = (int)((hi >> (8 * (i + 3))) & 0xFF);         // column cx+3 = byte 4+i+3
                // every 9-arc contains ring pixel k or k+8: both within +-t_lo -> never a corner
                const bool keep = !((abs(v - n) <= t_lo && abs(v - s) <= t_lo) || (abs(v - e) <= t_lo && abs(v - w) <= t_lo));
                keep4 |= keep ? (1u << i) : 0u;
            }
        }
        // survivors are rare: one ballot decides for the whole wave-row
        if (__ballot(keep4 != 0u) != 0ull) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const bool keep = (keep4 >> i) & 1u;
                const unsigned long long m = __ballot(keep);
                if (m != 0ull) {
                    int base = 0;
                    if (lane_id() == 0) base = atomicAdd(&nsurv, __popcll(m));
                    base = __shfl(base, 0, 64);
                    if (keep) surv[base + __popcll(m & lanemask_lt())] = (unsigned short)(py * ST_W + px + i);
                }
            }
        }
    }
    __syncthreads();
    const int ns = nsurv;
    for (int si = threadIdx.x; si < ns; si += 256) {
        const int pos = surv[si];
        const int cy = (pos >> 6) + 3, cx = (pos & 63) + 4;
        const int v = tile[cy][cx];
        int r[16];
        r[0] = tile[cy + 3][cx];      r[1] = tile[cy + 3][cx + 1];  r[2] = tile[cy + 2][cx + 2];
        r[3] = tile[cy + 1][cx + 3];  r[4] = tile[cy][cx + 3];      r[5] = tile[cy - 1][cx + 3];
        r[6] = tile[cy - 2][cx + 2];  r[7] = tile[cy - 3][cx + 1];  r[8] = tile[cy - 3][cx];
        r[9] = tile[cy - 3][cx - 1];  r[10] = tile[cy - 2][cx - 2]; r[11] = tile[cy - 1][cx - 3];
        r[12] = tile[cy][cx - 3];     r[13] = tile[cy + 1][cx - 3]; r[14] = tile[cy + 2][cx - 2];
        r[15] = tile[cy + 3][cx - 1];
        const int sc = fast_score16(v, r);
        if (sc >= t_lo && sc > 0) outt[pos >> 6][pos & 63] = (uint8_t)sc;
    }
    __syncthreads();
    for (int py = threadIdx.x >> 4; py < ST_H; py += 16) {
        const int gy = ty0 + py;
        if (gy < L.h && tx0 + px < L.spitch)
            *reinterpret_cast<unsigned*>(L.smap + (long long)f * L.splane + (long long)gy * L.spitch + tx0 + px) =
                reinterpret_cast<const unsigned*>(&outt[py][0])[px >> 2];
    }
}

// ------------------------------------------------------------------------------------------------
// k_cell_nms: one wave per FAST cell.  Reproduces, on the cell's sub-image, what
//   FAST(sub, iniThFAST, nms=true); if empty FAST(sub, minThFAST, nms=true)
// returns: detection area = sub-image minus a 3-px margin; scores of non-corners and of pixels
// outside the detection area count as 0; keep a corner iff its score is strictly greater than its 8
// neighbours'; output in row-major order.  Candidates go to the cell's slot range as
// score<<24 | y<<12 | x with x,y relative to minBorderX/Y (the coordinates of vToDistributeKeys).
#define NMS_PITCH 72      // interior starts at byte 4 of a row (dword aligned), zero ring at byte 3 and after the last column
#define NMS_ROWS 62       // cells are at most 65 px: 59 detection rows + 2 ring rows
#define NMS_WAVE_LDS (NMS_PITCH * NMS_ROWS)
__global__ __launch_bounds__(256) void k_cell_nms(const OrbGeom g, const OrbCell* __restrict__ cells,
                                                  unsigned* __restrict__ slots, int* __restrict__ cell_count)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[4][NMS_WAVE_LDS];
    const int wv = threadIdx.x >> 6, lane = lane_id();
    const int ci = blockIdx.x * 4 + wv;
    if (ci >= g.ncells) return;
    const int f = blockIdx.y + g.frame0;
    const OrbCell c = cells[ci];
    const OrbLevel& L = g.lv[c.level];
    const int rx0 = c.x0 + 3, ry0 = c.y0 + 3, rw = c.cw - 6, rh = c.ch - 6;
    int* count_out = cell_count + (long long)f * g.ncells + ci;
    if (rw <= 0 || rh <= 0) { if (lane == 0) *count_out = 0; return; }
    uint8_t* T = lds[wv];
    const uint8_t* sm = L.smap + (long long)f * L.splane;
    // rows 0 and rh+1 of the tile are the zero ring
    for (int i = lane; i < NMS_PITCH / 4; i += 64) {
        reinterpret_cast<unsigned*>(T)[i] = 0u;
        reinterpret_cast<unsigned*>(T + (rh + 1) * NMS_PITCH)[i] = 0u;
    }
    // interior: 16 lanes x 4 bytes per row (rw <= 59), 4 rows per step; bytes beyond rw are zeroed (they belong
    // to the neighbouring cell).  The score map has slack behind every plane, so the 4-byte over-read is safe.
    const int lx = (lane & 15) * 4, lrow = lane >> 4;
    bool any = false;
    {
        // all loads are issued before the first LDS store so that their latencies overlap (rh <= 59: 15 steps)
        unsigned v[15];
#pragma unroll
        for (int it = 0; it < 15; it++) {
            const int yy = 4 * it + lrow;
            v[it] = 0;
            if (yy < rh && lx < rw) __builtin_memcpy(&v[it], sm + (long long)(ry0 + yy) * L.spitch + rx0 + lx, 4);
        }
        const int valid = rw - lx;
        const unsigned keep_mask = valid >= 4 ? 0xFFFFFFFFu : (valid <= 0 ? 0u : (1u << (8 * valid)) - 1u);
#pragma unroll
        for (int it = 0; it < 15; it++) {
            const int yy = 4 * it + lrow;
            if (yy < rh) {
                const unsigned w = v[it] & keep_mask;
                *reinterpret_cast<unsigned*>(T + (yy + 1) * NMS_PITCH + 4 + lx) = w;
                if ((lane & 15) == 0) *reinterpret_cast<unsigned*>(T + (yy + 1) * NMS_PITCH) = 0u;   // left ring
                any |= w != 0u;
            }
        }
    }
    if (__ballot(any) == 0ull) { if (lane == 0) *count_out = 0; return; }      // no score >= min(ini,min) anywhere
    __builtin_amdgcn_s_waitcnt(0xc07f);     // lgkmcnt(0): this wave's LDS stores have landed
    __builtin_amdgcn_wave_barrier();
    unsigned* out = slots + (long long)f * g.slots_per_frame + c.slot_first;
    const int relx = rx0 - ORB_BORDER, rely = ry0 - ORB_BORDER;
    int n = 0;
    // two rows per step when a row fits 32 lanes; ballot bit order == row-major scan order
    const int rpi = rw <= 32 ? 2 : 1;
    const int xx = rpi == 2 ? (lane & 31) : lane, yoff = rpi == 2 ? (lane >> 5) : 0;
    // First iniThFAST; the fallback to minThFAST happens when FAST returned NO KEYPOINT, i.e. after
    // non-max suppression (:981) -- corners that suppress each other with equal scores also trigger it.
    for (int attempt = 0; attempt < 2 && n == 0; attempt++) {
        const int th = attempt == 0 ? g.ini_th : g.min_th;
        for (int y0 = 0; y0 < rh; y0 += rpi) {
            const int yy = y0 + yoff;
            bool keep = false;
            int s = 0;
            const uint8_t* p = &T[(min(yy, rh - 1) + 1) * NMS_PITCH + 4 + xx];
            if (yy < rh && xx < rw) s = p[0];
            // most rows hold no corner at all: skip the 8 neighbour reads for the whole wave
            if (__ballot(s >= th && s > 0) == 0ull) continue;
            {
                if (s >= th && s > 0) {
                    // scores below the threshold belong to non-corners and count as 0
#define NB(o) ((int)p[o] >= th ? (int)p[o] : 0)
                    keep = s > NB(-1) && s > NB(1) &&
                           s > NB(-NMS_PITCH - 1) && s > NB(-NMS_PITCH) && s > NB(-NMS_PITCH + 1) &&
                           s > NB(NMS_PITCH - 1) && s > NB(NMS_PITCH) && s > NB(NMS_PITCH + 1);
#undef NB
                }
            }
            const unsigned long long m = __ballot(keep);
            if (keep) {
                const int pos = n + __popcll(m & lanemask_lt());
                if (pos < c.slot_cap)
                    out[pos] = ((unsigned)s << 24) | ((unsigned)(rely + yy) << 12) | (unsigned)(relx + xx);
            }
            n += __popcll(m);
        }
    }
    if (lane == 0) *count_out = n;
}

void orb_launch_score(hipStream_t s, const OrbGeom& g_dev, int ntiles, int nframes)
{
    hipLaunchKernelGGL(k_fast_score, dim3(ntiles, nframes), dim3(256), 0, s, g_dev);
}
void orb_launch_nms(hipStream_t s, const OrbGeom& g_dev, const OrbCell* cells, int ncells, int nframes,
                    unsigned* slots, int* cell_count)
{
    hipLaunchKernelGGL(k_cell_nms, dim3((ncells + 3) / 4, nframes), dim3(256), 0, s, g_dev, cells, slots, cell_count);
}
