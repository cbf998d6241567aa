// mpt_internal.h -- what the host translation units of the map-point table share: mpt_host.cpp (the table itself and its refresh),
// mpt_fuse_host.cpp (Fuse on the table), mpt_sim3_host.cpp (ComputeSim3's two matchers on the table), mpt_track_host.cpp (SearchLocalPoints, TrackWithMotionModel) and frame_pose_host.cpp (the
// pose on table points).  Every call stages through the frame handles' block (FrameState::stage, frame_internal.h).
#pragma once
#include "frame_internal.h"
#include "mpt_types.h"

struct ccm_map_table {
    ccm_ctx* ctx = nullptr;                      // nullptr once the context is gone
    int capacity = 0;
    DevBuf mem;                                  // the columns, one block
    MptTable T{};
    DevBuf order; int n_order = 0; bool order_all = true;    // order_all: ascending slot over the LIVE slots
    int stamp = 0;                               // per-table call counter of SearchLocalPoints: seen[slot] == stamp <=> seen in this call
    std::vector<uint32_t> gen; std::vector<int32_t> row; uint32_t cur_gen = 0;   // host: last row of a slot within one update / order
    DevBuf where; unsigned fuse_stamp = 0;       // ccm_fuse_select_table_frames: per slot, stamp << 32 | position in that call's slot list
};

static inline int check_table(ccm_ctx* c, const ccm_map_table* t)
{
    if (!t->ctx) return ccm_fail(c, CCM_E_STATE, "map-point table outlived its context");
    if (t->ctx != c) return ccm_fail(c, CCM_E_ARG, "map-point table belongs to another context");
    return CCM_OK;
}

// Marks every slot of list [n] with its last position; CCM_E_ARG for a slot outside the table.  dup: whether a slot occurs twice.
static inline int mark_slots(ccm_ctx* c, ccm_map_table* t, int n, const int32_t* list, bool* dup)
{
    for (int r = 0; r < n; r++)
        if (list[r] < 0 || list[r] >= t->capacity) return ccm_fail(c, CCM_E_ARG, "slot %d (entry %d) outside [0, %d)", list[r], r, t->capacity);
    if (t->gen.empty()) { t->gen.assign(t->capacity, 0); t->row.assign(t->capacity, 0); }
    if (++t->cur_gen == 0) { std::fill(t->gen.begin(), t->gen.end(), 0); t->cur_gen = 1; }
    *dup = false;
    for (int r = 0; r < n; r++) {
        const int s = list[r];
        if (t->gen[s] == t->cur_gen) *dup = true;
        t->gen[s] = t->cur_gen; t->row[s] = r;
    }
    return CCM_OK;
}
