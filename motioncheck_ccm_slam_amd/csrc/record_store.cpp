// record_store.cpp -- the device half of the keyed record store (record_store.h).
#include "record_store.h"

RecordStore::~RecordStore()
{
    if (device < 0) return;
    (void)hipSetDevice(device);
    for (void* p : d_col) if (p) (void)hipFree(p);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    if (h_out) (void)hipHostFree(h_out);
}

int RecordStore::bind(ccm_ctx* c)
{
    CCM_HIP(c, hipSetDevice(c->device));
    device = c->device;
    int rc = rebuild(c, initial_cap);
    if (rc) return rc;
    ix.table_dirty = false;
    return CCM_OK;
}

// The old arena is freed once the copy has run.
int RecordStore::rebuild(ccm_ctx* c, int64_t new_cap)
{
    void* n_col[2] = { nullptr, nullptr };
    const size_t n = (size_t)std::max<int64_t>(new_cap, 1);
    h_jobs.reserve(ix.entry.size());
    if (hipMalloc(&n_col[0], n * ix.elem[0]) != hipSuccess) return ccm_fail(c, CCM_E_NOMEM, "%s: arena of %zu %s", name, n, unit);
    if (hipMalloc(&n_col[1], n * ix.elem[1]) != hipSuccess) { (void)hipFree(n_col[0]); return ccm_fail(c, CCM_E_NOMEM, "%s: arena of %zu %s", name, n, unit); }
    ix.plan_compaction(h_jobs);
    int rc = CCM_OK;
    if (!h_jobs.empty()) {
        rc = ccm_upload(c, d_jobs, h_jobs.data(), h_jobs.size() * sizeof(RecordMoveJob), c->stream);
        if (rc == CCM_OK) {
            move(c->stream, d_col, n_col, d_jobs.as<RecordMoveJob>(), (int)h_jobs.size());
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
                rc = ccm_fail(c, CCM_E_DEVICE, "%s: moving the arena failed", name);
        }
    }
    for (int k = 0; k < 2; k++) { if (d_col[k]) (void)hipFree(d_col[k]); d_col[k] = n_col[k]; }
    cap = (int64_t)n;
    return rc;
}

// Applies the pending inserts, replacements and erases: grows or compacts the arena when needed, appends the new records at its
// tail and brings the device's slot table up to date.  Everything is queued on c->stream.
int RecordStore::flush(ccm_ctx* c)
{
    const int64_t add = ix.pending_elements();
    const bool mostly_holes = ix.used - ix.live > ix.used / 2;
    if (!d_col[0] || mostly_holes || ix.used + add > cap) {
        int64_t new_cap = std::max(cap, initial_cap);
        if (ix.live + add > new_cap) new_cap = std::max(2 * cap, ix.live + add);
        int rc = rebuild(c, new_cap);
        if (rc) return rc;
    }
    if (!ix.pending.empty()) {
        const int64_t tail = ix.plan_flush(h_col);
        for (int k = 0; k < 2 && add; k++)
            CCM_HIP(c, hipMemcpyAsync(static_cast<char*>(d_col[k]) + (size_t)tail * ix.elem[k], h_col[k].data(), h_col[k].size(), hipMemcpyHostToDevice, c->stream));
    }
    if (ix.table_dirty) {
        ix.table(h_slot);
        int rc = ccm_upload(c, d_slot, h_slot.data(), h_slot.size() * sizeof(RecordSlot), c->stream);
        if (rc) return rc;
        ix.table_dirty = false;
    }
    return CCM_OK;
}

int RecordStore::landing(ccm_ctx* c, const char* who, size_t bytes)
{
    if (bytes <= h_out_cap) return CCM_OK;
    if (h_out) (void)hipHostFree(h_out);
    h_out = nullptr; h_out_cap = 0;
    const size_t want = bytes + bytes / 2 + 4096;
    if (hipHostMalloc(&h_out, want, hipHostMallocDefault) != hipSuccess) { h_out = nullptr; return ccm_fail(c, CCM_E_NOMEM, "%s: %zu bytes of page-locked memory", who, want); }
    h_out_cap = want;
    return CCM_OK;
}

int RecordStore::begin(ccm_ctx* c)
{
    CCM_HIP(c, hipSetDevice(c->device));
    for (int i = 0; i < 4; i++) if (!ev[i]) CCM_HIP(c, hipEventCreate(&ev[i]));
    return mark(c, 0);
}

void RecordStore::end()
{
    for (int i = 0; i < 3; i++) {
        float t = 0;
        last_ms[i] = hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess ? (double)t : 0.0;
    }
}

int RecordStore::keys(int capacity, int64_t* keys, int64_t* seq) const
{
    if (capacity < 0 || (capacity > 0 && !keys)) return CCM_E_ARG;
    if (ix.slots() > capacity) return CCM_E_CAPACITY;
    ix.keys(keys, seq);
    return ix.slots();
}

int RecordStore::arena(int64_t* capacity, int64_t* used, int64_t* live) const
{
    if (capacity) *capacity = cap;
    if (used) *used = ix.used;
    if (live) *live = ix.live;
    return CCM_OK;
}

int RecordStore::last_timing(double ms3[3]) const
{
    for (int i = 0; ms3 && i < 3; i++) ms3[i] = last_ms[i];
    return ms3 ? CCM_OK : CCM_E_ARG;
}
