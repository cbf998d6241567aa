// map_types.h -- what map_host.cpp hands to the launches of map_kernels.hip (ccm_create_new_map_points).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include "map_math.h"

#define MAP_TPB 256              // threads per block of all three kernels
#define MAP_TH_LOW 50            // ORBmatcher::TH_LOW
#define MAP_POS_BITS 20          // a node range holds fewer than 2^20 features (checked by the host: n <= 2^20 - 1)

// Per neighbour k: skipped by the baseline rule, F12, the epipole.  cam[0] is the current keyframe, cam[1 + k] neighbour k.
struct MapKf { int32_t skipped; float ex, ey; float F12[9]; };

struct MapDev {
    int32_t n1, n_kf;
    int32_t n_free, n_nodes;     // features of the current keyframe that take part in the match (no map point, a node); its distinct nodes
    float ratioFactor;           // 1.5f * mvScaleFactors[1] of the current keyframe (:307)
    // inputs
    const MapCam*  cam;          // [1 + n_kf]
    const MapKf*   kf;           // [n_kf]
    const MapFeat* f1;           // [n1]
    const uint8_t* desc1;        // [n1][32]
    const int32_t* cnode1;       // [n1] compact node id, -1 = no node, -2 = holds a map point
    const int32_t* free1;        // [n_free] the features with cnode1 >= 0, ascending
    const int32_t* range;        // [n_kf][n_nodes][2] first position and length of the node's features in the flattened side 2
    const MapFeat* f2;           // [m2] the neighbours' candidate features (no map point, a node of the current keyframe), neighbour-major,
    const uint8_t* desc2;        //      inside a neighbour by node and then by index: the order the reference visits them in
    const int32_t* idx2;         // [m2] index in the neighbour
    // per (k, i1), row k * n1 + i1
    int32_t* mpos;               // position in the flattened side 2 of the match, -1 = none (written for the features of free1 only)
    uint8_t* gate;               // the status before the resolution (MAP_OK = passes every gate)
    uint8_t* status;             // the final status
    float*   X;                  // [..][3]
    // the result list, room for n1 rows
    int32_t* first;              // [n_kf + 1]
    int32_t* out_kf; int32_t* out_idx1; int32_t* out_idx2; float* out_x3d;
};

// ---- ccm_create_new_map_points_frames: the keyframes are frame handles (frame_internal.h) and nothing of them is flattened per call.
// One keyframe as the three *_frames kernels read it: the handle's arrays by feature index, and its keyframe part -- the features
// that have a node ordered by (node, index), the directory of distinct nodes, and node-ordered copies of what the match reads.
struct MapKfView {
    const MapCam*  cam;
    const float*   kx; const float* ky; const int32_t* oct;    // [n]
    const int32_t* mp_id;        // [n] >= 0: the feature holds a map point
    const uint8_t* desc;         // [n][32]
    const float*   sf; const float* sig2;                      // mvScaleFactors, mvLevelSigma2
    const int32_t* node;         // [n]
    const int32_t* order;        // [first[n_nodes]] feature index at each position of the node order
    const int32_t* nodes;        // [n_nodes] ascending
    const int32_t* first;        // [n_nodes + 1]
    const MapFeat* feat_o;       // node-ordered MapFeat
    const uint8_t* desc_o;       // node-ordered descriptors
    int32_t n, n_nodes;
};
struct MapFramesDev {
    int32_t n1, n_kf;
    float ratioFactor;
    const MapKf*     kf;         // [n_kf]
    const MapKfView* view;       // [1 + n_kf]: the current keyframe, then the neighbours
    // per (k, i1), row k * n1 + i1
    int32_t* midx;               // the match: feature index in neighbour k, -1 = none (written for every row)
    uint8_t* gate; uint8_t* status; float* X;
    int32_t* first; int32_t* out_kf; int32_t* out_idx1; int32_t* out_idx2; float* out_x3d;
};

void map_match_launch(hipStream_t, const MapDev&);
void map_triangulate_launch(hipStream_t, const MapDev&);
void map_resolve_launch(hipStream_t, const MapDev&);
void map_frames_launch(hipStream_t, const MapFramesDev&);
