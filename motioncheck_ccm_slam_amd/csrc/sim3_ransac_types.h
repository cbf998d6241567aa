// sim3_ransac_types.h -- launch arguments and launcher of k_sim3_ransac, shared by sim3_ransac_host.cpp and sim3_ransac_kernels.hip.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#define S3R_TPB  256      // threads per workgroup (4 waves)
#define S3R_HPB  64       // hypotheses per workgroup: one lane of wave 0 each for the closed form
#define S3R_TILE 1024     // correspondences staged in LDS at a time (48 KB); larger solvers take several passes

struct S3rSolver {        // 64 bytes
    int32_t first, n;             // correspondences first .. first+n-1
    int32_t fix_scale;
    int32_t hyp_first, n_hyp;     // rows of the per-hypothesis outputs (and of draws)
    int32_t words;                // ceil(n / 64) mask words per hypothesis
    int64_t mask_first;           // first mask word of hypothesis 0
    float K1[4], K2[4];           // fx, fy, cx, cy
};
struct S3rBlock { int32_t solver, hyp0, n, pad; };   // hypotheses hyp0 .. hyp0+n-1 (n <= S3R_HPB) of one solver

struct S3rDev {
    const S3rSolver* solvers; const S3rBlock* blocks;
    const float* X1; const float* X2;                 // [..][3]
    const float* max_err1; const float* max_err2;
    const int32_t* draws;                             // [hypothesis][3]
    int32_t* count; int32_t* sample;                  // [hypothesis], [hypothesis][3]
    float* rts;                                       // [hypothesis][13]: R (9), t (3), s
    unsigned long long* mask;                         // inlier bits, correspondence i of a solver = bit i % 64 of word i / 64
};

void sim3_ransac_launch(hipStream_t, const S3rDev&, int n_blocks);
