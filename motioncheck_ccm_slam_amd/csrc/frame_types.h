// frame_types.h -- kernel argument structures, launch constants and launchers of frame_kernels.hip, shared with the host
// translation units of the frame handles (frame_host.cpp, mpt_host.cpp; through frame_internal.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "../../include/ccm_hot.h"
#include "map_math.h"
#include "undistort.h"

#define FB_TPB 1024

struct FrameBuildArgs {
    int n, cols, rows; float min_x, min_y, inv_w, inv_h;
    const ccm_keypoint* kps; const uint8_t* src_desc;  // gather source (an extracted image) or nullptr: x..desc already written
    int keep_xy;                                       // with kps: x / y were uploaded (undistorted), take only octave / angle / desc
    float* kx; float* ky; int* oct; float* angle; uint8_t* desc; int* cell_first; int* cell_items; int* mp_id;
};
// k_frame_build_batch: one record per frame in device memory (the frame's source rows of the extract, its count and the pointers into
// its block); what the frames of a call share travels in the kernel arguments.
struct FrameBatchRec {
    const ccm_keypoint* kps; const uint8_t* src_desc; int n, pad_;
    float* kx; float* ky; int* oct; float* angle; uint8_t* desc; int* cell_first; int* cell_items; int* mp_id;
};
struct FrameBatchArgs {
    const FrameBatchRec* rec;                          // [gridDim.x]
    int cols, rows; float min_x, min_y, inv_w, inv_h;
    int undistort;                                     // 0: the extracted coordinates (cam == NULL or k1 == 0), cam is not read
    UndistortCam cam;
};
// The points of the handle's map-point ids: xyz [n_mp][3] (the caller's array; pos and flags null), or the columns of a map-point
// table of capacity n_mp: pos [n_mp][3] float, widened (Converter::toVector3d of a float cv::Mat is exact), and flags, where a slot
// that is not CCM_MP_LIVE is a bad id.
struct PoseGatherArgs {
    int n; const float* kx; const float* ky; const int* oct; const int* mp_id;
    int n_mp; const double* xyz; const float* pos; const uint8_t* flags; const float* inv_sigma2; int n_levels;
    int* first; double* pts; double* obs; double* info; int* kof; int* status;
};
struct KfGatherArgs {
    int m; const int* order; const float* kx; const float* ky; const int* oct; const uint8_t* desc; const float* sf; const float* sig2;
    MapFeat* feat_o; uint8_t* desc_o;
};

size_t frame_build_lds(int cells);
int frame_launch_build(hipStream_t, const FrameBuildArgs&);
int frame_launch_build_batch(hipStream_t, int n_frames, const FrameBatchArgs&);
void frame_launch_prep_last(hipStream_t, int nq, const uint8_t* valid, const int* oct, const float* scale, float th, float* qr, int* minl, int* maxl);
void frame_launch_scatter_ids(hipStream_t, int n, const int* match, const int* src, const int* status, int* mp_id);
void frame_launch_pose_gather(hipStream_t, const PoseGatherArgs&);
void frame_launch_pose_scatter(hipStream_t, int n, const int* kof, const int* first, const uint8_t* outl, uint8_t* outlier);
void frame_launch_kf_gather(hipStream_t, const KfGatherArgs&);
