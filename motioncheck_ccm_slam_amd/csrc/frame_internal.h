// frame_internal.h -- what the host translation units of the frame handles share: frame_host.cpp (the handles), frame_window_host.cpp
// and frame_pose_host.cpp (their matchers and pose stage) and the mpt_*_host.cpp files (the map-point table and the calls that take a
// frame and a table).  The kernel argument structures and launchers they use come from the kernel files' types headers.
#pragma once
#include "staging.h"
#include "window_types.h"
#include "frame_types.h"
#include "pose_types.h"
#include "bow_directory_dev.h"

int orb_last_result(ccm_ctx*, const ccm_keypoint** kps, const uint8_t** desc, const int32_t** counts, int* n_images, int* max_per_image,
                    int* nlevels);

// What ccm_frame_compute_bow needs of a vocabulary (bow_host.cpp): its context, sizes, the host weights and the device flags
// "weight > 0" per node; and k_voc_transform on n descriptors in device memory (word, leaf, nid: device, [n] each).
struct VocView { ccm_ctx* ctx; int n_nodes, n_words; const double* weight; const uint8_t* pos_dev; };
VocView voc_view(const ccm_vocabulary*);
void voc_launch_transform(const ccm_vocabulary*, hipStream_t, const uint8_t* feat_dev, int n, int levelsup, int* word, int* leaf, int* nid);

struct FrameMem { DevBuf buf; };                 // one device block per frame, recycled through the context's pool

// Device layout of a frame (one block, 64-byte aligned segments): kx, ky [n] f32 | octave [n] i32 | angle [n] f32 |
// desc [n][32] | mp_id [n] i32 | cell_items [n] i32 | cell_first [cols*rows+1] i32.  The first five are what a host upload
// fills, in one copy.
struct ccm_frame {
    ccm_ctx* ctx = nullptr;                      // nullptr once the context is gone
    FrameMem* mem = nullptr;
    int n = 0, cols = 0, rows = 0, n_levels = 0; // n_levels: octaves are in [0, n_levels)
    float min_x = 0, min_y = 0, inv_w = 0, inv_h = 0;
    bool has_angle = false;
    float* kx = nullptr; float* ky = nullptr; int* oct = nullptr; float* angle = nullptr; uint8_t* desc = nullptr;
    int* mp_id = nullptr; int* cell_items = nullptr; int* cell_first = nullptr;
    // ---- the keyframe part (ccm_frame_set_bow / _camera / _pose), a second block taken on the first setter.  Layout: node [n] |
    // order [n] | nodes [n] | first [n + 1] (one upload per set_bow) | feat_o [n] MapFeat | desc_o [n][32] (node-ordered copies,
    // gathered on the device once bow and camera are both there) | sf, sig2 [kMaxLevels] | cam.
    static const int kMaxLevels = 256;           // ccm_frame_create admits octaves up to 255
    FrameMem* kf_mem = nullptr;
    bool has_bow = false, has_cam = false, has_pose = false;
    int n_bow = 0, n_nodes = 0, cam_levels = 0;  // features with a node; distinct nodes; n_levels of set_camera
    float sf1 = 0;                               // scale_factors[1] (ratioFactor of CreateNewMapPoints, :307)
    MapCam cam = {};                             // host copy of *d_cam: set_camera writes the intrinsics, set_pose Tcw and Ow
    int* node = nullptr; int* order = nullptr; int* nodes = nullptr; int* first = nullptr;
    MapFeat* feat_o = nullptr; uint8_t* desc_o = nullptr; float* sf = nullptr; float* sig2 = nullptr; MapCam* d_cam = nullptr;
};

struct FrameState {
    std::vector<FrameMem*> pool;                 // free blocks
    std::vector<FrameMem*> kf_pool;              // free blocks of keyframe parts
    std::vector<ccm_frame*> live;
    Staging stage{ true };                       // per-call staging of every call on handles and tables; the setters leave uploads queued
    DevBuf ci, cd, cn, ev, pts, obs, info, err, outl, kof, first;
    std::vector<struct ccm_map_table*> tables;   // map-point tables of this context (mpt_internal.h)
    DevBuf slp;                                  // SearchLocalPoints: per-entry temporaries, workgroup counts and offsets
    DevBuf fuse;                                 // ccm_fuse_select_table_frames: membership flags, the compact query list, its selections;
                                                 // the work area of the two calls of mpt_sim3_host.cpp as well
    DevBuf tmm;                                  // ccm_frame_track_motion_model: the queries made from the last frame (radius, levels, flags, descriptors)
    double slp_ms[3] = { -1, 0, 0 };            // host wall time of its last call (ccm_frame_search_local_points_timing)
};

// The handle's features and grid as the windowed matchers read them
static inline WinGrid frame_win_grid(const ccm_frame* f)
{
    return WinGrid{ f->n, f->cols, f->rows, f->min_x, f->min_y, f->inv_w, f->inv_h, f->kx, f->ky, f->oct, f->desc, f->cell_first, f->cell_items };
}

// A per-level table of a kernel argument or staging segment: src [n] and zeros up to CCM_MAX_LEVELS
static inline void fill_levels(float* dst, const float* src, int n) { for (int l = 0; l < CCM_MAX_LEVELS; l++) dst[l] = l < n ? src[l] : 0.f; }

// ccm_destroy: releases the device memory of the map-point tables still alive and orphans their handles (mpt_host.cpp)
void mpt_tables_orphan(FrameState* S);
// The context's frame state, created on first use.
FrameState* frame_state(ccm_ctx* c);
// device -> pageable host, then wait for the stream (rare paths: fallbacks, test taps)
int frame_fetch(ccm_ctx* c, void* dst, const void* src_dev, size_t bytes);
// CCM_E_ARG for a handle of another context or one that outlived its context
int frame_check(ccm_ctx* c, const ccm_frame* f);
// A handle passed under a name of the caller's (printf-style, e.g. "kfs[%d]", k): CCM_E_ARG for a null handle or one of another context,
// `orphaned` (CCM_E_STATE, or CCM_E_ARG where the entry point has always answered so) for one that outlived its context
int frame_named_check(ccm_ctx* c, const ccm_frame* f, int orphaned, const char* fn, const char* who, ...) __attribute__((format(printf, 5, 6)));
// The handle's keyframe block (the layout above), taken from the pool on the first setter; nothing when it has one (frame_host.cpp)
int kf_block(ccm_ctx* c, ccm_frame* f);
// What a handle lacks to serve as a keyframe of CreateNewMapPoints ("bow", "camera", "pose"), or nullptr
const char* frame_keyframe_lacks(const ccm_frame* f);

// One windowed-matcher call whose queries already lie in device memory: the candidate lists with their capacity retry, the
// single-workgroup acceptance kernel (or the host acceptance loops) and the scatter of the new map-point ids into the handle.
// status / out / flag lie in the staging block at o_status / o_out / o_flag, inside [0, res_end): the results come back
// with one download of that range.  out must hold -1 and flag the occupancy flags when the call is made.
struct WinDevCall {
    int mode, nq;
    const float* qx; const float* qy; const float* qr; const int* minl; const int* maxl;
    const uint8_t* qdesc; const uint8_t* act; const uint8_t* qflag;
    const int* id_src;                           // new id of query q (nullptr: q itself)
    const float* qang;                           // mode 2 with check_ori: the query side's angles (device)
    size_t o_status, o_out, o_flag, res_end;
    float nnratio; int orb_dist, check_ori;
    // host copies for the host acceptance loops; nullptr: act / qflag / the occupancy flags are fetched from the device there
    const uint8_t* h_act; const uint8_t* h_qflag; const float* h_qang; const ccm_frame* last;
    int* ids_copy;                               // optional second target of the id scatter (a copy of mp_id in io), or nullptr
    bool host_accept;                            // out: the host acceptance loops ran (nothing of [0, res_end) was downloaded)
};
// occupied [n] in/out and match [n] out are host arrays; returns nmatches or an error.
int frame_window_dev(ccm_ctx* c, ccm_frame* f, WinDevCall& w, uint8_t* occupied, int32_t* match);

// Optimizer::PoseOptimizationClient(Frame&) on a handle whose arguments the entry point has checked (f->n > 0): the points are
// mp_xyz [n_mp][3] (host, uploaded with the call) or, with mp_xyz == nullptr, the device columns pos / flags of a map-point table of
// capacity n_mp.  Staging [ n_inliers+status | outlier | pose | intr | inv_sigma2 | (xyz) ]: one upload, gather -> pose_launch ->
// scatter, one download.  A bad id or octave sets *bad_id and leaves pose7 / outlier / n_inliers alone: the caller words the error.
int frame_pose_run(ccm_ctx* c, ccm_frame* f, int n_mp, const double* mp_xyz, const float* pos, const uint8_t* flags,
                   const float* inv_level_sigma2, int n_levels, const double intr[4], double pose7[7], uint8_t* outlier, int32_t* n_inliers,
                   bool* bad_id);
// Its device half, for a caller that keeps the pose in a staging layout of its own (ccm_frame_track_motion_model): gather -> pose_launch ->
// scatter queued on blocks of io the caller has filled.  ninl: 16 bytes, [0] n_inliers, [1] the bad-id status; outl [n]; pose 56 bytes,
// in/out; intr 32 bytes; is2 [n_levels] float; xyz [n_mp][3] double, read only when pos == nullptr.  Nothing is copied or awaited.
struct PoseIo { size_t ninl, outl, pose, intr, is2, xyz; };
int frame_pose_queue(ccm_ctx* c, ccm_frame* f, int n_mp, const float* pos, const uint8_t* flags, int n_levels, const PoseIo& o);
