// mpt_device.h -- device functions the kernels on the map-point table share (mpt_kernels.hip, reloc_kernels.hip): the projection of a
// table row and MapPoint::PredictScale, in the arithmetic of float cv::Mat expressions.
#pragma once
#include <hip/hip_runtime.h>

// The projection SearchLocalPoints, TrackWithMotionModel's SearchByProjection(Current, Last) and the relocalisation SearchByProjection
// use (src/Frame.cpp:150-163, src/ORBmatcher.cpp:1380-1396, :1503-1511): Pc = Rcw P + tcw summed in double and stored as float, invz =
// 1 / PcZ, u = fx * PcX * invz + cx in float, left to right, every operation rounded (the build's -ffp-contract=off keeps the compiler
// from fusing them).  What rejects a point behind the camera differs between the callers and stays with them.
__device__ inline void mpt_to_camera(const float* Tcw, const float* P, float* Pc)
{
    for (int r = 0; r < 3; r++)
        Pc[r] = (float)((double)Tcw[4 * r] * (double)P[0] + (double)Tcw[4 * r + 1] * (double)P[1] + (double)Tcw[4 * r + 2] * (double)P[2] +
                        (double)Tcw[4 * r + 3]);
}
__device__ inline void mpt_pinhole(float fx, float fy, float cx, float cy, const float* Pc, float invz, float& u, float& v)
{
    u = fx * Pc[0] * invz + cx;
    v = fy * Pc[1] * invz + cy;
}

// MapPoint::PredictScale (src/MapPoint.cpp:837-852 for a keyframe, :854-869 for a frame) with the raw mfMaxDistance, the expression
// slp_in_frustum ends with: the double log rounded to float, ceilf, clamped; a NaN gives 0
__device__ inline int fuse_predict_level(float max_d, float dist, float log_scale, int n_levels)
{
    const float ratio = max_d / dist;
    const float lg = (float)log((double)ratio);
    const float q = ceilf(lg / log_scale);
    return !(q >= 0.0f) ? 0 : (q >= (float)n_levels ? n_levels - 1 : (int)q);
}
