// sim3_frames_types.h -- kernel argument structures and launchers of mpt_sim3_opt_kernels.hip: the gathers in front of k_sim3_ransac
// and k_sim3_opt for correspondences named by features of two keyframe handles, and the list and scatter kernels of
// ccm_compute_sim3_table_frames.  Shared with sim3_ransac_host.cpp, mpt_sim3_host.cpp and mpt_sim3_opt_host.cpp.
#pragma once
#include "mpt_types.h"
#include "sim3_types.h"
#include "sim3_ransac_types.h"

#define S3G_TPB 256        // the gathers and the scatter: one thread per correspondence, the pair uniform per workgroup (blockIdx.y)
#define S3L_TPB 256        // k_sim3_chain_list: one workgroup per pair walks its side-1 features in order, 4 waves at a time

// What the gathers read of one pair: both poses as rows of [R | t] and, of either handle, the feature count and the device pointers
// to its undistorted keypoints, octaves and map-point slots
struct Sim3FramesPair {
    float T1w[12], T2w[12];
    int n1, n2;
    const float* kx1; const float* ky1; const int* oct1; const int* mp1;
    const float* kx2; const float* ky2; const int* oct2; const int* mp2;
};

// k_sim3_solver_gather (ccm_sim3_solver_create_frames): correspondence e of solver k = (feature1[e] of kf1, feature2[e] of kf2)
struct Sim3SolverGather {
    const Sim3FramesPair* pairs; const S3rSolver* solvers;
    const int* feature1; const int* feature2;
    int n_levels1, n_levels2; const float* max_err_level1; const float* max_err_level2;      // [n_levels] device tables
    float* X1; float* X2; float* max_err1; float* max_err2;
    int* status;                                 // [0]: a correspondence that names no feature, no LIVE slot or no level
};
void sim3_solver_gather_launch(hipStream_t, const Sim3SolverGather&, const MptTable&, int n_solvers, int max_n);

// k_sim3_opt_gather (ccm_optimize_sim3_table_frames, ccm_compute_sim3_table_frames): correspondence e of problem k, first[k] <= e <
// first[k + 1] with first in device memory, = (feature1[e], feature2[e]); the six arrays of Sim3Dev
struct Sim3OptGather {
    const Sim3FramesPair* pairs; const int* first;
    const int* feature1; const int* feature2;
    int n_levels1, n_levels2; const float* inv_level_sigma2_1; const float* inv_level_sigma2_2;
    double* P1; double* P2; double* obs1; double* obs2; double* info1; double* info2;
    int* status;
};
// max_n: no problem has more correspondences
void sim3_opt_gather_launch(hipStream_t, const Sim3OptGather&, const MptTable&, int n_problems, int max_n);

// ccm_compute_sim3_table_frames between k_sim3_agree and k_sim3_opt_gather: the correspondence list of every pair in ascending i1,
// dense over the pairs
struct Sim3ChainArgs {
    int n_pairs, n_rows;                         // n_rows: the features of every side 1, the most rows the list can take
    const Sim3Pair* pairs; const Sim3FramesPair* views;
    const int* matched12; const int* matched_idx2; const int* match12;       // flat over side 1
    int* cnt;                                    // [n_pairs] correspondences of a pair
    int* first;                                  // [n_pairs + 1] its first row
    int* feature1; int* feature2;                // the rows
};
// k_sim3_chain_list counting, k_sim3_chain_prefix, k_sim3_chain_list placing
void sim3_chain_list_launch(hipStream_t, const Sim3ChainArgs&, const MptTable&);
// pruned[first1 + feature1[e]] = 1 for the rows e with inlier[e] == 0 (pruned cleared by the caller)
void sim3_chain_scatter_launch(hipStream_t, const Sim3ChainArgs&, int max_n1, const uint8_t* inlier, uint8_t* pruned);
