// pose_types.h -- kernel argument structure and launcher of pose_kernels.hip, shared with pose_host.cpp and the frame handles
// (frame_internal.h).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#define PO_TPB 256

struct PoseDev {
    int n_frames;
    double* poses;            // [n_frames][7] in/out
    const double* intr;       // [n_frames][4]
    const int* first;         // [n_frames+1]
    const double* pts;        // [total][3]
    const double* obs;        // [total][2]
    const double* info;       // [total]
    double* err;              // [total][2] scratch: last computed error per edge
    uint8_t* outlier;         // [total] out
    int* n_inliers;           // [n_frames] out
};
void pose_launch(hipStream_t, const PoseDev&);
