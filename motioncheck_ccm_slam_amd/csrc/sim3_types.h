// sim3_types.h -- kernel argument structure and launcher of sim3_kernels.hip, shared with sim3_host.cpp.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#define S3_TPB 256

struct Sim3Dev {
    int n_problems;
    double* sim3;             // [n][8] in/out: qx,qy,qz,qw, tx,ty,tz, s
    const int* fix_scale;     // [n]
    const double* K1; const double* K2;     // [n][4] fx, fy, cx, cy
    const int* first;         // [n+1]
    const double* P1; const double* P2;     // [total][3] map points in their own camera frame
    const double* obs1; const double* obs2; // [total][2]
    const double* info1; const double* info2;
    const float* th2;         // [n]
    double* err;              // [total][4] scratch: last computed e12, e21
    uint8_t* inlier;          // [total] out
    int* n_in;                // [n] out
};
void sim3_launch(hipStream_t, const Sim3Dev&);
