// reloc_types.h -- kernel argument structures and launchers of reloc_kernels.hip, shared with reloc_host.cpp: the relocalisation
// overload of ORBmatcher::SearchByProjection (src/ORBmatcher.cpp:1478-1605) on a frame handle, a keyframe handle and the map-point table.
#pragma once
#include "mpt_types.h"

#define RLC_TPB 256        // k_reloc_project: one thread per keyframe feature

// What k_reloc_project reads of the keyframe, the caller's view of the current frame and the found set, and the matcher's queries it
// writes.  The view is uniform per launch and travels in the kernel arguments.
struct RelocArgs {
    int n_kf; const int* kf_id;                      // the keyframe's map-point ids (table slots)
    const unsigned long long* where; unsigned stamp; // found set: where[slot] >> 32 == stamp
    const float* cam;                                // Tcw [12], Ow [3] in device memory, or nullptr: the two below
    float Tcw[12], Ow[3], fx, fy, cx, cy, min_x, max_x, min_y, max_y, log_scale, th;
    int n_levels; float scale[CCM_MAX_LEVELS];
    // per keyframe feature: the queries (qx / qy / level / act are also the taps)
    float* qx; float* qy; float* qr; int* minl; int* maxl; int* level; uint8_t* act; uint8_t* qflag; uint8_t* qdesc;
    int* head;                                       // [0]: an id outside the table or of a slot that is not LIVE
};

// where[id] = stamp << 32 for every id of ids [n] inside the table (an explicit found list, or the current frame's own ids)
void reloc_launch_mark(hipStream_t, int n, const int* ids, int capacity, unsigned long long* where, unsigned stamp);
// k_reloc_project: the queries of SearchByProjection(CurrentFrame, pKF, sAlreadyFound) from the keyframe's ids and the table
void reloc_launch_project(hipStream_t, const RelocArgs&, const MptTable&);
// before the search: out = -1, flag = (mp_id >= 0), ids_out = mp_id [n_cur]; with head[0] set every query is switched off (act [n_kf] = 0)
void reloc_launch_clear(hipStream_t, int n_cur, int n_kf, const int* head, const int* mp_id, int* out, uint8_t* flag, int* ids_out, uint8_t* act);

// ---- ccm_frame_relocalize_candidate
// cam = Tcw [12], Ow [3] of pose7 (ba_pose_to_camera), one thread: the view of a search behind a pose stage, without a read-back
void reloc_launch_camera(hipStream_t, const double* pose7, float* cam);
// mp_id[feature[j]] = slot[j] for the PnP inliers (the host has checked the features: inside the frame, each once)
void reloc_launch_set(hipStream_t, int n_matched, const int* feature, const int* slot, int n_cur, int* mp_id);
// behind a pose stage: with ninl[1] == 0 (no bad id) and ninl[0] >= discard_from the features with outlier != 0 lose their id
void reloc_launch_discard(hipStream_t, int n, int* mp_id, const uint8_t* outlier, const int* ninl, int discard_from);
