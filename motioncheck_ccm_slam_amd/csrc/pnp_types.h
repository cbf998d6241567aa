// pnp_types.h -- launch arguments and launchers of k_pnp_hypotheses and k_pnp_refine, shared by pnp_host.cpp and pnp_kernels.hip.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#define PNP_TPB    256    // threads per workgroup of k_pnp_hypotheses (4 waves)
#define PNP_HPB    16     // hypotheses per workgroup: one lane of wave 0 each, its two 12x12 matrices in LDS ([element][lane], 36 KB)
#define PNP_TILE   1024   // correspondences staged in LDS at a time (24 KB); larger solvers take several passes
#define PNP_MAXSET 8      // largest mRansacMinSet
#define PNP_RTPB   64     // k_pnp_refine: one wave per (solver, record)

struct PnpSolver {        // 64 bytes
    int32_t first, n;             // correspondences first .. first+n-1
    int32_t hyp_first, n_hyp;     // rows of the per-hypothesis outputs
    int32_t words;                // ceil(n / 64) mask words per hypothesis
    int32_t min_set;
    int64_t mask_first;           // first mask word of hypothesis 0
    float K[4];                   // fx, fy, cx, cy
    int32_t pad[4];
};
struct PnpBlock { int32_t solver, hyp0, n, pad; };    // hypotheses hyp0 .. hyp0+n-1 (n <= PNP_HPB) of one solver
struct PnpRecord {                                    // one Refine(): the inlier set of hypothesis hyp of a solver
    int32_t solver, hyp;
    int32_t row, pad;             // row of the refinement outputs
    int64_t mask_first;           // first word of its refined mask
};

struct PnpDev {
    const PnpSolver* solvers; const PnpBlock* blocks;
    const float* P2D; const float* P3D;               // [..][2], [..][3]
    const float* max_err;                             // mvMaxError
    const int32_t* sample;                            // [hypothesis][PNP_MAXSET] correspondence indices of the minimal set
    int32_t* count;                                   // [hypothesis]
    double* Rt;                                       // [hypothesis][12]: R (9, row-major), t (3)
    unsigned long long* mask;                         // inlier bits, correspondence i of a solver = bit i % 64 of word i / 64
    double* detail;                                   // [hypothesis][PNP_DETAIL] or null
};
struct PnpRefineDev {
    const PnpSolver* solvers; const PnpRecord* records;
    const float* P2D; const float* P3D; const float* max_err;
    const unsigned long long* hyp_mask;               // the masks k_pnp_hypotheses wrote
    int32_t* count; double* Rt; unsigned long long* mask; double* detail;      // per record
};

// k_pnp_gather (ccm_pnp_solver_create_frames): correspondence e = (feature[e] of a frame handle, slot[e] of a map-point table)
#define PNP_GTPB   256
struct PnpGather {
    int32_t n, n_cur, capacity, n_levels;             // correspondences; features of the frame; slots of the table; entries of sigma2
    float th2;
    const int32_t* feature; const int32_t* slot;
    const float* kx; const float* ky; const int* oct; // the frame handle's columns
    const float* pos; const uint8_t* flags;           // the table's columns
    const float* sigma2;                              // mvLevelSigma2, [CCM_MAX_LEVELS] in device memory
    float* P2D; float* P3D; float* max_err;           // what PnpDev reads
    int32_t* status;                                  // [0] raised by a correspondence that cannot be gathered
};

void pnp_gather_launch(hipStream_t, const PnpGather&);
void pnp_hypotheses_launch(hipStream_t, const PnpDev&, int n_blocks);
void pnp_refine_launch(hipStream_t, const PnpRefineDev&, int n_records);
