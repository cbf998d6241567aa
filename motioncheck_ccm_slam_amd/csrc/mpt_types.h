// mpt_types.h -- kernel argument structures and launchers of the map-point table, shared by the mpt_*.hip kernel files and the
// mpt_*_host.cpp files that launch them.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include "../../include/ccm_hot.h"

#define SLP_TPB 256        // k_slp_frustum / k_slp_compact: 4 waves per workgroup
#define SCAN_TPB 1024
#define MPR_TPB 256        // k_mpt_refresh: one wave per map point, 4 points per workgroup
#define FUSE_TPB 256       // k_fuse_project: one thread per (keyframe, point) pair, the keyframe uniform per workgroup
#define TMM_TPB 256        // k_tmm_project / k_tmm_discard: one thread per feature
#define MPR_LDS_ROWS 256   // descriptors a wave keeps in LDS: 8 KB per wave, 32 KB per workgroup; further rows are read from global memory

struct MptTable {                                // the table's columns (device)
    int capacity;
    float* pos; float* normal; float* min_dist; float* max_dist; uint8_t* desc; uint8_t* flags; int* seen;
};

struct SlpArgs {
    int n_order; const int* order;               // order == nullptr: entry j is slot j
    int stamp;
    float Tcw[12], Ow[3], fx, fy, cx, cy, min_x, max_x, min_y, max_y, cos_limit, log_scale;
    int n_levels; float scale[CCM_MAX_LEVELS]; float th;
    // per list entry (written where the entry is in view) and per wave / workgroup
    float* tmp_u; float* tmp_v; float* tmp_vc; int* tmp_level; unsigned long long* mask; int* wg_cnt; int* wg_off;
    // per entry in view, in list order: the matcher's queries (qx / qy are also the taps mTrackProjX / Y) and the taps
    float* qx; float* qy; float* qr; int* minl; int* maxl; uint8_t* qdesc; uint8_t* qact; uint8_t* qflag; int* slots;
    int* tap_level; float* tap_vc;
};

// What k_mpt_refresh reads of a keyframe handle: device pointers the handle owns (Ow: d_cam->Ow; sf: kMaxLevels floats, zero-padded).
struct MptKfView { const uint8_t* desc; const float* Ow; const int* oct; const float* sf; int n_levels; int pad_; };

struct MptRefreshArgs {
    int n, what;                                 // what: CCM_MPR_*
    const int* slot; const int* obs_first; const int* obs_kf; const int* obs_feat; const int* ref_kf; const int* ref_feat;
    const float* pos; const uint8_t* flags;      // optional rows written first
    const MptKfView* view;
    int* best; float* normal; float* min_dist; float* max_dist;      // per listed point, in the call's result block
};

// ---- mpt_correct_kernels.hip: ccm_map_table_correct_frames
// What the three kernels read and write of keyframe k: cam = &d_cam->Tcw of the handle, Tcw [12] then Ow [3] (nullptr for a handle
// without a keyframe block, which the host lets no point read); oct and sf as in MptKfView.
struct MptCorrectKf { float* cam; const int* oct; const float* sf; int n_levels; int pad_; };
#define MPC_CAM_STRIDE 16  // floats per moved keyframe in cam_new: Tcw [12], Ow [3], one unused

struct MptCorrectArgs {
    int n_points, n_moved, transform, order;     // CCM_MC_*
    const int* slot; const int* owner;
    const int* obs_first; const int* obs_kf; const int* obs_feat; const int* ref_kf; const int* ref_feat;   // obs_first == nullptr: no normal / depth
    const double* sim3_before; const double* sim3_after;        // SIM3: [n_moved][8]
    const float* Tcw_after; const float* Ow_after;              // RIGID: [n_moved][12], [n_moved][3]
    const MptCorrectKf* kf;                                     // [n_kf], the moved ones first
    float* cam_new;                                             // [n_moved][MPC_CAM_STRIDE], written by k_mpt_correct_poses
    float* pos; float* normal; float* min_dist; float* max_dist;     // per listed point, in the call's result block
};
// k_mpt_correct_poses (the moved keyframes' new Tcw / Ow into cam_new), k_mpt_correct (the points, reading the handles' old cameras)
// and k_mpt_correct_publish (cam_new into the handles), in this order on one stream
void mpt_launch_correct(hipStream_t, const MptCorrectArgs&, const MptTable&);

// ccm_fuse_select_table_frames.  What k_fuse_project reads of keyframe k: the caller's pose and camera and the handle's map-point ids.
struct FuseView { float Tcw[12], Ow[3], fx, fy, cx, cy, min_x, max_x, min_y, max_y; int n; int pad_; const int* mp_id; };

struct FuseArgs {
    int n_kf, n_points;
    const FuseView* views; const int* slot; const uint8_t* skip;     // skip == nullptr: no point is skipped
    unsigned long long* where; unsigned stamp;                       // per table slot: stamp << 32 | position in the slot list
    uint8_t* held;                                                   // [n_kf][n_points] keyframe k holds point j
    float log_scale; int n_levels; float scale[CCM_MAX_LEVELS]; float th;
    // per pair, in the call's result block
    int* best_idx; int* best_dist; uint8_t* gate; float* u; float* v; int* level;
    // the pairs that passed every gate, in no particular order: the queries of k_window_select and their pair index
    int* cnt; float* qx; float* qy; float* qr; int* minl; int* maxl; int* qkf; int* qpair; uint8_t* qdesc;
};

// ccm_frame_track_motion_model: what k_tmm_project reads of the last frame and the caller's camera, and the matcher's queries it writes
struct TmmArgs {
    int n_last; const int* last_id; const uint8_t* last_outlier;     // last_outlier == nullptr: none
    float Tcw[12], fx, fy, cx, cy, min_x, max_x, min_y, max_y;
    float* qx; float* qy; uint8_t* act; uint8_t* qflag; uint8_t* qdesc;   // per last-frame feature; qx / qy / act are also the taps
    int* head;                                                       // [0]: an id outside the table or of a slot that is not LIVE
};

// k_tmm_project: the queries of SearchByProjection(Current, Last) from the last frame's ids and the table
void tmm_launch_project(hipStream_t, const TmmArgs&, const MptTable&);
// before a search pass: out = -1, flag = 0 [n_cur]; mp_id = -1, or with head[0] set the ids kept and act [n_last] = 0
void tmm_launch_clear(hipStream_t, int n_cur, int n_last, const int* head, int* mp_id, int* out, uint8_t* flag, uint8_t* act);
// the outliers (nullptr: none) lose their id; ids_out = mp_id afterwards; head[1] += features that keep a slot with HAS_OBS
void tmm_launch_discard(hipStream_t, int n, int* mp_id, const uint8_t* outlier, const MptTable&, int* ids_out, int* head);
void mpt_launch_scatter(hipStream_t, const MptTable&, int n, const int* slot, const float* pos, const float* normal, const float* min_dist,
                        const float* max_dist, const uint8_t* desc, const uint8_t* flags);
void mpt_launch_gather(hipStream_t, const MptTable&, int n, const int* slot, float* pos, float* normal, float* min_dist, float* max_dist,
                       uint8_t* desc, uint8_t* flags, int* seen);
void slp_launch_mark(hipStream_t, const MptTable&, int n, const int* mp_id, int stamp, int* ids, uint8_t* occ, int* match, int* cnt);
int  slp_workgroups(int n_order);
// k_slp_frustum, k_slp_scan (cnt[0] = entries in view) and k_slp_compact
void slp_launch_frustum(hipStream_t, const SlpArgs&, const MptTable&, int* cnt);
void mpt_launch_refresh(hipStream_t, const MptRefreshArgs&, const MptTable&);
// k_fuse_where and k_fuse_held (max_n: the largest feature count among the keyframes), then k_fuse_project: gates, taps, cnt[0] queries
void fuse_launch_project(hipStream_t, const FuseArgs&, const MptTable&, int max_n);
// k_fuse_where and k_fuse_held alone: held [n_kf][n_points] (cleared by the caller) for the views' mp_id and the slot list
void fuse_launch_membership(hipStream_t, const FuseArgs&, const MptTable&, int max_n);

// ---- mpt_sim3_kernels.hip: ccm_search_by_sim3_table_frames and ccm_search_by_projection_table_frames
#define SIM3_TPB 256       // k_sim3_project: one thread per (pair, direction, feature), pair and direction uniform per workgroup
#define LOOP_TPB 256       // k_loop_project: one thread per (view, point), the view uniform per workgroup

// What k_sim3_project reads of one direction of one pair: the source side's pose and ids, the Sim3 into the target, the intrinsics
// (pKF1's for both directions), the target's bounds, feature count and levels
struct Sim3View {
    float Tsw[12], Sts[12], fx, fy, cx, cy, min_x, max_x, min_y, max_y;
    int n, n_target, e0, side_t;                 // source / target feature counts; first flat entry; target side (0: kf1, 1: kf2)
    const int* mp_id; const int* mark_i; const uint8_t* mark_b;      // MATCHED: mark_i[i] >= 0 (direction 1 -> 2) or mark_b[i] (2 -> 1)
};
struct Sim3Args {
    int n_views, n_entries;                      // 2 * n_pairs; features of every side-1 handle, then of every side-2 handle
    const Sim3View* views;
    float log_scale[2]; int n_levels[2]; float scale[2][CCM_MAX_LEVELS]; float th;
    int* sel; uint8_t* gate; float* u; float* v; int* level;         // per entry; gate / u / v / level may be nullptr
    int* cnt; float* qx; float* qy; float* qr; int* minl; int* maxl; int* qview; int* qent; uint8_t* qdesc;   // the query list
};
// vbAlreadyMatched2 of pair p: am2[first2[p] + matched_idx2[i]] = 1 for the marked features i of side 1
struct Sim3Pair { int n1, n2, first1, first2; };
void sim3_launch_marks(hipStream_t, int n_pairs, int max_n1, const Sim3Pair* pairs, const int* matched12, const int* matched_idx2, uint8_t* am2);
void sim3_launch_project(hipStream_t, const Sim3Args&, const MptTable&, int max_n);
// match12[i1] = sel1[i1] where sel2[sel1[i1]] == i1 (sel2 = sel + n_side1)
void sim3_launch_agree(hipStream_t, int n_pairs, int max_n1, const Sim3Pair* pairs, const int* sel, int n_side1, int* match12);

struct LoopArgs {
    int n_kf, n_points;
    const FuseView* views; const int* slot;
    const uint8_t* held; const uint8_t* found;   // [n_kf][n_points] from the where[] lookups
    float log_scale; int n_levels; float scale[CCM_MAX_LEVELS]; float th;
    // per pair, in list order: the queries of k_window_candidates / k_window_greedy and the taps
    float* qx; float* qy; float* qr; int* none; int* qkf; int* qlevel; uint8_t* act; uint8_t* qdesc; int* out;
    uint8_t* gate; float* u; float* v; int* level;
};
// per (view, feature): flag = matched_slot >= 0, oct (the views' octaves in one array), ms_out = matched_slot, found[k][position of
// matched_slot in the list] = 1 by the stamped where[] of the table
void loop_launch_marks(hipStream_t, int n_kf, int n_points, int max_n, const struct WinGrid* grids, const int* feat_first, const int* matched_slot,
                       const unsigned long long* where, unsigned stamp, int capacity, uint8_t* flag, int* oct, int* ms_out, uint8_t* found);
void loop_launch_project(hipStream_t, const LoopArgs&, const MptTable&);
// after the acceptance: matched_slot[best_idx] = slot for the accepted points that are not observed; best_dist (optional)
void loop_launch_finish(hipStream_t, int n_kf, int n_points, const struct WinGrid* grids, const int* feat_first, const int* slot, const int* out,
                        const uint8_t* held, const MptTable&, int* ms_out, int* best_dist);
// best_idx / best_dist of query q to pair qpair[q]
void fuse_launch_scatter(hipStream_t, int nq, int n_pairs, const int* qpair, const int* sel_i, const int* sel_d, int* best_idx, int* best_dist);
