// orb_types.h -- device-visible geometry tables of the ORB pipeline and the launchers of its CDNA4 (gfx950) kernels, shared with orb_host.cpp.
//
// Pipeline per batch (all frames of the batch in every launch), one file per stage:
//   orb_pyramid.hip      k_pyr_resize  x (nlevels-1)   cv::resize INTER_LINEAR 8u                                ORBextractor.cpp:1293
//   orb_fast_cells.hip   k_fast_cells                  FAST-9/16 score + per-cell threshold choice + 3x3 NMS,    :957-998, :978-984 (cv::FAST)
//                                                      fused on cell-row bands (scores stay in LDS)
//   orb_fast_tiles.hip   k_fast_score + k_cell_nms     the same in two kernels through a score map, for cells wider than one LDS tile
//   orb_octree.hip       k_octree                      DistributeOctTree                                         :707-931
//   orb_orient_desc.hip  k_orient_desc                 IC_Angle + 7x7 blur + rBRIEF                              :68-95, :1259, :100-316
// orb_device.h holds the device helpers that more than one stage uses.  Wavefront = 64 everywhere; ballots are 64-bit.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "../../include/ccm_hot.h"

#define ORB_MAX_LEVELS 16
#define ORB_EDGE 19            // EDGE_THRESHOLD, cslam/src/ORBextractor.cpp:65
#define ORB_BORDER 16          // EDGE_THRESHOLD-3 = minBorderX/Y, :941
#define ORB_HALF_PATCH 15
#define ORB_MAX_ROOTS 8
#define ORB_PATCH_R 21         // 18 (max rotated pattern offset) + 3 (blur taps)
#define ORB_PATCH_D 43
#define ORB_BLUR_D 37

struct OrbLevel {
    // level pixels: img + frame*plane + y*pitch + x.  Level 0 points at the caller's images.
    const uint8_t* img; long long plane; int pitch;
    int w, h;
    // FAST score map, same indexing
    uint8_t* smap; long long splane; int spitch;
    // bilinear tables that make this level from level-1 (device pointers; unused for level 0)
    const int* xofs; const short* xab; const int* yofs; const short* yab;
    // FAST cells of this level inside OrbGeom::cells
    int cell_first, ncells;
    // score tiles (64x16) of this level inside the flattened tile index space
    int tile_first, tiles_x, tiles_y;
    // DistributeOctTree inputs
    int quota;                 // mnFeaturesPerLevel[level]
    int roots; float hx;       // nIni, hX (ORBextractor.cpp:711-713)
    int bw, bh;                // maxBorder-minBorder extents
    int key_first, key_cap;    // per-frame candidate scratch (ping-pong) range
    int out_first, out_cap;    // per-frame selected-keypoint slots
    float scale;               // mvScaleFactor[level]
    float kp_size;             // (int)(PATCH_SIZE*scale)
};

struct OrbCell {
    short level, x0, y0, cw, ch, pad;   // sub-image rectangle passed to FAST (:978)
    int slot_first, slot_cap;           // per-frame candidate slots of this cell
};

// Constants of the order in which k_fast_cells's waves take the items of the rejection test (the functions: orb_device.h, fc_enum).
struct FcEnum {
    short n_dw, d_step, r_step, pad_;  // detection dwords per row (>= 0); FC_ITEM_STRIDE % n_dw, FC_ITEM_STRIDE / n_dw
    unsigned nd_inv;                   // floor(2^20 / n_dw) + 1: i / n_dw by multiply-shift, exact for i < 2^20 / n_dw (i < FC_ITEM_STRIDE here)
};

// A band of k_fast_cells: consecutive cells of one cell row of one level, with everything the kernel needs before it can request the
// band's pixels -- one 64-byte scalar load.  (Until round 3 the kernel loaded a 16-byte band record, THEN the level record it
// pointed to, THEN the first and last cell records, and computed two integer reciprocals: 3,700 cycles of dependent scalar work in
// front of the pixel loads of a workgroup that lives 26,000.)
struct OrbBand {
    const uint8_t* img;                // level image base; nullptr for level 0, whose pointer, pitch and plane change per call (OrbGeom::lv[0])
    long long plane;                   // bytes per frame of the level image
    int lpitch, w, h;                  // level pitch and size
    int level;
    int cell_first, ncells;            // consecutive cells of one row of one level
    short xa, y0, pitch, bh;           // tile origin (xa multiple of 4, one spare dword left of the first cell), LDS pitch, rows
    short c_lo, c_hi, dw_lo, dw_hi;    // detection columns of the tile [c_lo, c_hi); dwords with a detection column and both neighbours
    unsigned pw_inv, pq_inv;           // floor(2^20 / (pitch / 4)) + 1, floor(2^20 / (pitch / 16)) + 1: i / PW and i / PQ by multiply-shift
    // its (at most ORB_BAND_CELLS) cells: first detection column of the tile and number of detection columns, candidate slots of the cell
    short clo[4], cwd[4];
    int slot_first[4], slot_cap[4];
    FcEnum items;                      // the rejection test's item enumeration over dwords dw_lo .. dw_hi
    int pad_[1];
};
#define ORB_BAND_CELLS 4
static_assert(sizeof(OrbBand) == 128, "two s_load_dwordx16");

struct OrbGeom {
    int nlevels, ncells, ntiles;
    int frame0;              // first frame of this launch: kernels index frame blockIdx + frame0 (chunked host-buffer pipeline)
    int ini_th, min_th;
    int slots_per_frame;     // sum of slot_cap
    int keys_per_frame;      // sum of key_cap
    int out_per_frame;       // sum of out_cap
    int list_cap;            // max(quota)+4: node-list capacity of the octree kernel
    int umax[16];
    OrbLevel lv[ORB_MAX_LEVELS];
};
static_assert(sizeof(OrbGeom) <= 3584, "OrbGeom is passed by value in the kernel arguments (4 KiB limit)");

extern "C" hipError_t orb_upload_pattern();
size_t orb_octree_lds_bytes(int list_cap);
void orb_launch_resize(hipStream_t, const OrbGeom&, int level, int dw, int dh, int nframes, int* clear_status);
void orb_launch_score(hipStream_t, const OrbGeom&, int ntiles, int nframes);
void orb_launch_nms(hipStream_t, const OrbGeom&, const OrbCell*, int ncells, int nframes, unsigned* slots, int* cell_count);
void orb_launch_fast_cells(hipStream_t, const OrbGeom&, const OrbCell*, const OrbBand*, int nbands, int nframes, size_t lds_bytes,
                           unsigned* slots, int* cell_count, int* clear_status);
size_t orb_fast_cells_lds(int pitch, int bh);
void orb_launch_octree(hipStream_t, const OrbGeom&, const OrbCell*, int nlevels, int nframes, int list_cap,
                       const unsigned* slots, const int* cell_count, unsigned* keysA, unsigned* keysB,
                       unsigned* out, int* out_count, int* status);
void orb_launch_orient_desc(hipStream_t, const OrbGeom&, int out_per_frame, int nframes, const unsigned* sel,
                            const int* sel_count, ccm_keypoint* kps, uint8_t* desc, int* counts, int max_per_image,
                            int* status);
void orb_launch_od_steer_debug(hipStream_t, const int* m01, const int* m10, int n, float* angle_deg, float* ab, int8_t* offs);
