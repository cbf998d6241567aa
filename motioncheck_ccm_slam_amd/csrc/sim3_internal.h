// sim3_internal.h -- what the array routes of ComputeSim3's solver and optimiser (sim3_ransac_host.cpp, sim3_host.cpp) share with the
// routes on keyframe handles and the map-point table (mpt_sim3_opt_host.cpp): the contexts' device buffers, so that both routes of a
// context use one set, and the body of the two solver constructors.
#pragma once
#include "staging.h"
#include "sim3_types.h"
#include "sim3_ransac_types.h"
#include "sim3_frames_types.h"

// ccm_optimize_sim3 / ccm_optimize_sim3_table_frames / ccm_compute_sim3_table_frames: the arrays k_sim3_opt reads and writes.  The
// array route uploads all of them; the routes on handles fill P1 .. i2 with k_sim3_opt_gather and keep the small ones in the frame
// handles' staging block.
struct Sim3State { DevBuf sim3, fix, K1, K2, first, P1, P2, o1, o2, i1, i2, th2, err, inl, nin; };

// The staging area (staging.h) of the batched Sim3Solver, laid out [inputs | outputs]: one upload, one launch, one download per batch.
struct Sim3RansacState { Staging stage{ false }; };

// Where the correspondences of ccm_sim3_solver_create_frames come from: feature1 / feature2 [first[n_solvers]] name a feature of the
// pair's two handles (pairs: [n_solvers], as the kernel reads them); k_sim3_solver_gather fills the X1 / X2 / max_err1 / max_err2
// segments from them and the table's columns.  pb then carries no X1 / X2 / max_err1 / max_err2, and indices1 = feature1.
struct Sim3SolverFrames {
    MptTable T; const Sim3FramesPair* pairs; const int32_t* feature1; const int32_t* feature2;
    const float* max_err_level1; const float* max_err_level2; int n_levels1, n_levels2;
};
// The body of both create calls (fr == nullptr: the correspondences are the caller's arrays), under the caller's ccm_guard.
int sim3_solver_create_body(ccm_ctx* c, const ccm_sim3_ransac_problem* pb, const Sim3SolverFrames* fr, ccm_sim3_solver** out);
