// mpt_internal.h -- what the host translation units of the map-point table share: mpt_host.cpp (the table itself and its refresh),
// mpt_fuse_host.cpp (Fuse on the table), mpt_sim3_host.cpp (ComputeSim3's two matchers on the table), mpt_sim3_opt_host.cpp (its solver, optimiser and chain), mpt_correct_host.cpp (loop and
// merge corrections), mpt_track_host.cpp (SearchLocalPoints,
// TrackWithMotionModel) and frame_pose_host.cpp (the pose on table points).  Every call stages through the frame handles' block (FrameState::stage, frame_internal.h).
#pragma once
#include "frame_internal.h"
#include "mpt_types.h"
#include "sim3_frames_types.h"
#include <atomic>
#include <memory>
#include <mutex>
#include <shared_mutex>

// The rows of a table: the shared columns pos | normal | min_dist | max_dist | desc | flags (and, in the same block, the `seen` column
// of the handle that created them).  Every handle on them (ccm_map_table_create, ccm_map_table_attach) holds one reference; the memory
// goes with the last one.  Handles of several contexts, each on a thread of its own, may name the same rows:
//   mu       a call whose kernels write a shared column (ccm_map_table_update, _refresh, _correct_frames) holds it exclusively from entry to return, a
//            call that only reads them holds it shared; the handle count changes under the exclusive lock
//   written  "last unsynchronised write": recorded on the writer's stream when a writing call returns with its kernels still queued
//            and the rows have more than one handle; a call of another context makes its stream wait for it before it queues anything
//   writer   the context that recorded `written`, nullptr when nothing is pending (read under either lock, changed under the exclusive one)
// Reading calls return synchronised (they download their result), so a writer finds no reader's work queued on the rows.
struct MptRows {
    int device = 0, capacity = 0;
    DevBuf mem;                                  // the columns, one block
    MptTable T{};                                // seen: the creating handle's column
    std::shared_mutex mu;
    hipEvent_t written = nullptr;
    ccm_ctx* writer = nullptr;
    std::atomic<int> handles{ 0 };
    ~MptRows() { if (written) (void)hipEventDestroy(written); }
};

struct ccm_map_table {
    ccm_ctx* ctx = nullptr;                      // nullptr once the context is gone
    int capacity = 0;
    std::shared_ptr<MptRows> rows;               // empty once the context is gone
    MptTable T{};                                // the rows' columns and this handle's seen
    DevBuf seen_mem;                             // a view's own seen column (the creating handle's lies in the rows' block)
    DevBuf order; int n_order = 0; bool order_all = true;    // order_all: ascending slot over the LIVE slots
    int stamp = 0;                               // per-handle call counter of SearchLocalPoints: seen[slot] == stamp <=> seen in this call
    std::vector<uint32_t> gen; std::vector<int32_t> row; uint32_t cur_gen = 0;   // host: last row of a slot within one update / order
    DevBuf where; unsigned fuse_stamp = 0;       // ccm_fuse_select_table_frames: per slot, stamp << 32 | position in that call's slot list
};

static inline int check_table(ccm_ctx* c, const ccm_map_table* t)
{
    if (!t->ctx) return ccm_fail(c, CCM_E_STATE, "map-point table outlived its context");
    if (t->ctx != c) return ccm_fail(c, CCM_E_ARG, "map-point table belongs to another context");
    return CCM_OK;
}

// The lock a table call holds on its rows, taken inside ccm_guard (a failing lock throws) and held from there to the return.  A call
// names one table, so there is no lock order.
struct RowsLock {
    ccm_ctx* c; MptRows* R; const bool write; bool synced = false;       // synced stays false when the body throws
    RowsLock(ccm_ctx* ctx, ccm_map_table* t, bool writes) : c(ctx), R(t->rows.get()), write(writes)
    {
        if (write) R->mu.lock(); else R->mu.lock_shared();
    }
    // Another context's unsynchronised write runs before whatever this call queues
    int wait()
    {
        if (!R->writer || R->writer == c) return CCM_OK;
        CCM_HIP(c, hipSetDevice(c->device));     // the body has not run yet
        CCM_HIP(c, hipStreamWaitEvent(c->stream, R->written, 0));
        return CCM_OK;
    }
    // synced: the call waited for its stream after its last launch.  A reading call always has when it succeeds; one that failed between
    // a launch and its wait may have left work queued on the rows, which the next writer must not overtake.
    ~RowsLock()
    {
        const bool shared = R->handles.load() > 1;       // an unshared table records nothing and waits for nothing
        if (!write) {
            if (!synced && shared) (void)hipStreamSynchronize(c->stream);
            R->mu.unlock_shared();
            return;
        }
        if (synced) R->writer = nullptr;
        else if (shared) {
            bool ok = R->written || hipEventCreateWithFlags(&R->written, hipEventDisableTiming) == hipSuccess;
            ok = ok && hipEventRecord(R->written, c->stream) == hipSuccess;
            if (!ok) { (void)hipGetLastError(); (void)hipStreamSynchronize(c->stream); }      // no event: nothing may stay pending
            R->writer = ok ? c : nullptr;
        }
        R->mu.unlock();
    }
    RowsLock(const RowsLock&) = delete; RowsLock& operator=(const RowsLock&) = delete;
};

// An entry point's body under ccm_guard and the lock on the table's rows.  write: its kernels write a shared column.  A reading body
// returns synchronised unless it fails; a writing body sets *synced when it waited for its stream behind its last launch.
template <class F> int table_call(ccm_ctx* c, ccm_map_table* t, bool write, const char* name, F&& body, const bool* synced = nullptr)
{
    return ccm_guard(c, name, [&]() -> int {
        RowsLock L(c, t, write);
        int rc = L.wait();
        if (rc) return rc;
        rc = body();
        L.synced = rc >= 0 && (write ? synced && *synced : true);
        return rc;
    });
}

// The table's stamped where[] (per slot: stamp << 32 | position in that call's slot list): created on first use, where every entry is
// older than any stamp, and cleared when the 32-bit stamp wraps.  Gives the stamp of this call.
static inline int next_where_stamp(ccm_ctx* c, ccm_map_table* t, hipStream_t st, unsigned* stamp)
{
    if (!t->where.p) {
        CCM_RESERVE(c, t->where, (size_t)t->capacity * 8);
        CCM_HIP(c, hipMemsetAsync(t->where.p, 0, (size_t)t->capacity * 8, st));
        t->fuse_stamp = 0;
    }
    if (t->fuse_stamp == 0xffffffffu) { CCM_HIP(c, hipMemsetAsync(t->where.p, 0, (size_t)t->capacity * 8, st)); t->fuse_stamp = 0; }
    *stamp = ++t->fuse_stamp;
    return CCM_OK;
}

// A view of the caller's as the Fuse and loop kernels read it
static inline void fuse_view_fill(FuseView& D, const ccm_fuse_view& V)
{
    std::memcpy(D.Tcw, V.Tcw, sizeof D.Tcw); std::memcpy(D.Ow, V.Ow, sizeof D.Ow);
    D.fx = V.fx; D.fy = V.fy; D.cx = V.cx; D.cy = V.cy; D.min_x = V.min_x; D.max_x = V.max_x; D.min_y = V.min_y; D.max_y = V.max_y;
    D.n = V.kf->n; D.pad_ = 0; D.mp_id = V.kf->mp_id;
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

// What the gathers of mpt_sim3_opt_kernels.hip read of a pair of the caller's
static inline Sim3FramesPair sim3_frames_pair(const ccm_frame* k1, const ccm_frame* k2, const float* T1w, const float* T2w)
{
    Sim3FramesPair V{};
    std::memcpy(V.T1w, T1w, sizeof V.T1w); std::memcpy(V.T2w, T2w, sizeof V.T2w);
    V.n1 = k1->n; V.n2 = k2->n;
    V.kx1 = k1->kx; V.ky1 = k1->ky; V.oct1 = k1->oct; V.mp1 = k1->mp_id;
    V.kx2 = k2->kx; V.ky2 = k2->ky; V.oct2 = k2->oct; V.mp2 = k2->mp_id;
    return V;
}

// What ccm_compute_sim3_table_frames (mpt_sim3_opt_host.cpp) hangs on the pipeline of ccm_search_by_sim3_table_frames (mpt_sim3_host.cpp):
// a segment of its own in the result part and in the input part of the staging block and in the work area, the launches behind
// k_sim3_agree, and the delivery after the one download.  The search lays the block out, uploads and downloads; the chain says how
// much it needs (size) and works inside its segments.
struct Sim3Chain {
    const ccm_compute_sim3_problem* p; ccm_compute_sim3_result* r;
    int n_pairs = 0; size_t sum1 = 0;
    size_t res_bytes = 0, in_bytes = 0, work_bytes = 0;
    size_t r_pruned = 0, r_first = 0, r_nin = 0, r_status = 0, r_f1 = 0, r_f2 = 0, r_inl = 0;         // offsets inside the segments
    size_t i_sim3 = 0, i_K1 = 0, i_K2 = 0, i_fix = 0, i_th2 = 0, i_view = 0, i_t1 = 0, i_t2 = 0, w_cnt = 0, w_f1 = 0, w_f2 = 0, w_inl = 0;
    void size(int n_pairs, size_t sum1);
    void fill(Staging& G, size_t o_in) const;                                  // the inputs, before the upload
    // everything from the list to the scatter, and the download of sim3; nothing is awaited
    int queue(ccm_ctx* c, const MptTable& T, Staging& G, size_t o_res, size_t o_in, uint8_t* work, int max_n1, const Sim3Pair* d_pair,
              const int* d_matched12, const int* d_matched_idx2, const int* d_match12) const;
    int deliver(ccm_ctx* c, const Staging& G, size_t o_res, size_t o_in) const;
    void none() const;                                                         // a call without a feature on either side
};
// What ccm_search_by_sim3_table_frames refuses before it takes the lock (n_pairs == 0 passes), and its body under the lock, with the chain (or nullptr) behind the agreement kernel
int sim3_search_check(ccm_ctx* c, const ccm_map_table* t, const ccm_sim3_search_problem* p, const ccm_sim3_search_result* r, const char* fn);
int sim3_search_run(ccm_ctx* c, ccm_map_table* t, const ccm_sim3_search_problem* p, ccm_sim3_search_result* r, const char* fn, Sim3Chain* chain);
