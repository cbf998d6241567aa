// ba_table.h -- what ba_table_host.cpp (the entry point ccm_ba_solve_table_frames: checks, staging, table lock) and ba_host.cpp (the
// solve) share: the source and the sink of a bundle adjustment whose observations, information values and points lie in keyframe
// handles and a map-point table.
#pragma once
#include "staging.h"
#include "ba_types.h"

// Filled by the entry point before the solve; the staging block G is reserved with this layout, 64-byte segments:
//   [0, res_end)          results, one download: pose7 [P][7] f64 | outlier bytes [E] | pos_out [L][3] f32
//   [in_begin, in_end)    inputs, one upload: pose7 | intr [P][4] f64 | slot [L] | edge_feat [E] (written by the solve, once the
//                         device's edge order is known) | BaTableKf [P] | level table | publish [P]
struct BaTableRoute {
    Staging* G = nullptr;
    size_t o_pose_out = 0, o_outl = 0, o_pos = 0, res_end = 0, in_begin = 0, o_pose_in = 0, o_intr = 0, o_feat = 0, in_end = 0;
    const int32_t* obs_feat = nullptr;     // [E] the caller's list (host), in the caller's edge order
    float* pos_out = nullptr;              // [L][3] the caller's, or nullptr
    BaTableArgs A{};                       // the entry point fills kf, slot, level_info, n_levels, publish, table_pos, pos_out; the solve the rest
    bool wrote = false;                    // out: the table and the published handles were written (false: no LM iteration ran)
};

// ccm_ba_solve on the problem `pb` describes (points, obs and info are nullptr) with `route` as source and sink.  One rank only.
int ba_solve_table(ccm_ctx* c, ccm_ba_problem* pb, const ccm_ba_options* opt, ccm_ba_result* res, BaTableRoute* route);
