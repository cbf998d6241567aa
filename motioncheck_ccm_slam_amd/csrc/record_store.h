// record_store.h -- the keyed record store under the KeyFrameDatabase (kfdb_host.cpp) and the covisibility index (covis_host.cpp):
// the bookkeeping of record_index.h plus its device half -- the arena of two columns, the slot table, the move jobs, the upload
// staging, the page-locked landing block of the owner's download and the four events of a query.  The owner holds its mutex around
// every call; the store's own entry points of the C ABI (size, slot, slots, keys, arena, last_timing) are the methods below.
#pragma once
#include "ccm_internal.h"
#include "record_index.h"

// Launches the owner's move kernel: n_jobs records from the columns src[0], src[1] into dst[0], dst[1].
typedef void (*RecordMoveFn)(hipStream_t s, const void* const src[2], void* const dst[2], const RecordMoveJob* job, int n_jobs);

struct RecordStore {
    RecordIndex ix;
    const char* const name;                 // the entry point that flushes, for failure texts
    const char* const unit;                 // what an element is called there ("words", "features")
    const RecordMoveFn move;
    int device = -1;                        // -1: not bound to a device yet; then there is no arena and arena() gives (0, 0, 0)
    int64_t initial_cap = 0;
    // ---- device side, touched by queries only (from the flush to the end of the download)
    void* d_col[2] = { nullptr, nullptr };  // the arena
    int64_t cap = 0;                        // elements allocated (tail and live elements: ix.used, ix.live)
    DevBuf d_slot, d_jobs;
    void* h_out = nullptr; size_t h_out_cap = 0;                  // page-locked landing block of the download
    std::vector<uint8_t> h_col[2];                                // upload staging: alive until the query's synchronise
    std::vector<RecordSlot> h_slot; std::vector<RecordMoveJob> h_jobs;
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };    // created by the first query
    double last_ms[3] = { 0, 0, 0 };        // flush, kernels, download of the last query

    RecordStore(size_t elem0, size_t elem1, const char* name_, const char* unit_, RecordMoveFn move_) : ix(elem0, elem1), name(name_), unit(unit_), move(move_) {}
    RecordStore(const RecordStore&) = delete; RecordStore& operator=(const RecordStore&) = delete;
    ~RecordStore();                                                // releases what lives on `device`

    int bind(ccm_ctx* c);                                          // at create: the store is on c's device, with an arena of initial_cap
    int rebuild(ccm_ctx* c, int64_t new_cap);                      // the uploaded live records, packed, into a new arena
    int flush(ccm_ctx* c);                                         // pending records and the slot table to the device, on c->stream
    int landing(ccm_ctx* c, const char* who, size_t bytes);        // h_out holds at least `bytes`
    int begin(ccm_ctx* c);                                         // a query starts: the events exist, the first is recorded
    int mark(ccm_ctx* c, int i) { CCM_HIP(c, hipEventRecord(ev[i], c->stream)); return CCM_OK; }      // 1: kernels, 2: download, 3: end
    void end();                                                    // after the synchronise: last_ms

    int keys(int capacity, int64_t* keys, int64_t* seq) const;
    int arena(int64_t* capacity, int64_t* used, int64_t* live) const;
    int last_timing(double ms3[3]) const;
};
