// covis_host.cpp -- C ABI of the device covisibility index (include/ccm_hot.h, section "Covisibility"): the store of one record per
// keyframe (table slot and octave per feature), the batched query that replaces the counter of KeyFrame::UpdateConnections
// (src/KeyFrame.cpp:644-662) and the observer loop of LocalMapping::KeyFrameCullingV3 (src/Mapping.cpp:818-855), and the ordered
// remainder of UpdateConnections replayed on the host over one row of weights (ccm_covis_connections, :664-711).  The store follows
// kfdb_host.cpp: host bookkeeping under a mutex, a pending list, an arena that a query grows and compacts.
#include "ccm_internal.h"
#include "mpt_internal.h"
#include "covis_types.h"
#include <cstdlib>
#include <memory>
#include <mutex>
#include <unordered_map>

static_assert(COVIS_MP_LIVE == CCM_MP_LIVE && COVIS_MP_BAD == CCM_MP_BAD, "covis_types.h mirrors CCM_MP_*");

namespace {

struct CovisEntry {                         // one slot, host side
    int64_t key = 0, seq = -1;              // seq < 0: free slot
    int64_t off = -1;                       // place in the arena; -1 while the record waits in `pending`
    int32_t len = 0;
};

struct CovisPending { int32_t slot; std::vector<int32_t> slots; std::vector<uint8_t> octave; };

int covis_lds_features()
{
    static const int v = [] {
        int n = COVIS_LDS_FEATURES;
        if (const char* e = std::getenv("CCM_COVIS_LDS_FEATURES")) {
            char* end = nullptr;
            const long x = std::strtol(e, &end, 10);
            if (end != e && x >= 0 && x < n) n = (int)x;
        }
        return n;
    }();
    return v;
}

int covis_cells(int len)                    // a power of two >= max(2 * len, 64)
{
    int64_t c = 64;
    while (c < 2 * (int64_t)len) c <<= 1;
    return (int)c;
}

}  // namespace

struct ccm_covis {
    int device = -1;                        // -1: not bound to a device yet (created without a context)
    int64_t initial_cap = 0;
    std::mutex mu;
    // ---- host bookkeeping (put / erase / clear touch nothing else)
    std::unordered_map<int64_t, int32_t> slot_of;
    std::vector<CovisEntry> entry;          // [slots]: its size is the high-water mark
    std::vector<int32_t> free_slots;
    std::vector<CovisPending> pending;      // put since the last flush, in put order
    int64_t next_seq = 0;
    bool table_dirty = false;               // the device's slot table is behind `entry`
    // ---- device side, touched by queries only (under mu, from the flush to the end of the download)
    int32_t* d_slots = nullptr; uint8_t* d_octave = nullptr;
    int64_t cap = 0, used = 0, live = 0;    // arena features: allocated, tail, held by uploaded live records
    DevBuf d_slot, d_jobs, d_q, d_hash, d_out;                    // d_out: [weights n_q x n_slots | n_mps | n_redundant | skipped]
    void* h_out = nullptr; size_t h_out_cap = 0;                  // page-locked landing block of the download
    std::vector<int32_t> h_slots; std::vector<uint8_t> h_octave;  // upload staging: alive until the query's synchronise
    std::vector<CovisSlot> h_slot; std::vector<CovisMoveJob> h_jobs; std::vector<CovisQ> h_q;
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };    // created by the first query
    double last_ms[3] = { 0, 0, 0 };        // flush, kernels, download of the last query (ccm_covis_last_timing)
};

namespace {

// Moves the uploaded live records, packed, into a new arena of new_cap features; the old one is freed once the copy has run.
int covis_rebuild(ccm_ctx* c, ccm_covis* d, int64_t new_cap)
{
    int32_t* n_slots = nullptr; uint8_t* n_octave = nullptr;
    const size_t feats = (size_t)std::max<int64_t>(new_cap, 1);
    if (hipMalloc(&n_slots, feats * 4) != hipSuccess) return ccm_fail(c, CCM_E_NOMEM, "ccm_covis_query: arena of %zu features", feats);
    if (hipMalloc(&n_octave, feats) != hipSuccess) { (void)hipFree(n_slots); return ccm_fail(c, CCM_E_NOMEM, "ccm_covis_query: arena of %zu features", feats); }
    d->h_jobs.clear();
    int64_t tail = 0;
    for (CovisEntry& e : d->entry) {
        if (e.seq < 0 || e.off < 0) continue;
        if (e.len > 0) d->h_jobs.push_back(CovisMoveJob{ e.off, tail, e.len, 0 });
        e.off = tail; tail += e.len;
    }
    int rc = CCM_OK;
    if (!d->h_jobs.empty()) {
        rc = ccm_upload(c, d->d_jobs, d->h_jobs.data(), d->h_jobs.size() * sizeof(CovisMoveJob), c->stream);
        if (rc == CCM_OK) {
            covis_launch_move(c->stream, CovisMove{ d->d_slots, d->d_octave, n_slots, n_octave, d->d_jobs.as<CovisMoveJob>(), (int32_t)d->h_jobs.size() });
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
                rc = ccm_fail(c, CCM_E_DEVICE, "ccm_covis_query: moving the arena failed");
        }
    }
    if (d->d_slots) (void)hipFree(d->d_slots);
    if (d->d_octave) (void)hipFree(d->d_octave);
    d->d_slots = n_slots; d->d_octave = n_octave; d->cap = (int64_t)feats; d->used = d->live = tail; d->table_dirty = true;
    return rc;
}

// Applies the pending puts and erases: grows or compacts the arena when needed, appends the new records at its tail and brings the
// device's slot table up to date.  Everything is queued on c->stream.
int covis_flush(ccm_ctx* c, ccm_covis* d)
{
    int64_t add = 0;
    for (const CovisPending& p : d->pending) add += (int64_t)p.slots.size();
    const bool mostly_holes = d->used - d->live > d->used / 2;
    if (!d->d_slots || mostly_holes || d->used + add > d->cap) {
        int64_t new_cap = std::max(d->cap, d->initial_cap);
        if (d->live + add > new_cap) new_cap = std::max(2 * d->cap, d->live + add);
        int rc = covis_rebuild(c, d, new_cap);
        if (rc) return rc;
    }
    if (!d->pending.empty()) {
        d->h_slots.clear(); d->h_octave.clear();
        const int64_t tail = d->used;
        for (const CovisPending& p : d->pending) {
            CovisEntry& e = d->entry[p.slot];
            e.off = tail + (int64_t)d->h_slots.size();
            d->h_slots.insert(d->h_slots.end(), p.slots.begin(), p.slots.end());
            d->h_octave.insert(d->h_octave.end(), p.octave.begin(), p.octave.end());
        }
        d->pending.clear();
        d->used += add; d->live += add; d->table_dirty = true;
        if (add) {
            CCM_HIP(c, hipMemcpyAsync(d->d_slots + tail, d->h_slots.data(), (size_t)add * 4, hipMemcpyHostToDevice, c->stream));
            CCM_HIP(c, hipMemcpyAsync(d->d_octave + tail, d->h_octave.data(), (size_t)add, hipMemcpyHostToDevice, c->stream));
        }
    }
    if (d->table_dirty) {
        d->h_slot.resize(d->entry.size());
        for (size_t s = 0; s < d->entry.size(); s++) {
            const CovisEntry& e = d->entry[s];
            d->h_slot[s] = e.seq < 0 ? CovisSlot{ 0, -1, 0 } : CovisSlot{ e.off, e.len, 0 };
        }
        int rc = ccm_upload(c, d->d_slot, d->h_slot.data(), d->h_slot.size() * sizeof(CovisSlot), c->stream);
        if (rc) return rc;
        d->table_dirty = false;
    }
    return CCM_OK;
}

double covis_ms(hipEvent_t a, hipEvent_t b) { float t = 0; return hipEventElapsedTime(&t, a, b) == hipSuccess ? (double)t : 0.0; }

// Under d->mu and, with a table, the shared lock on its rows.  q_slot: the queries' slot numbers, already looked up.
int covis_run(ccm_ctx* c, ccm_covis* d, ccm_map_table* t, const std::vector<int32_t>& q_slot, int what, int capacity, ccm_covis_result* r)
{
    const char* name = "ccm_covis_query";
    const int n_q = (int)q_slot.size(), n_slots = (int)d->entry.size();
    CCM_HIP(c, hipSetDevice(c->device));
    hipEvent_t* ev = d->ev;
    for (int i = 0; i < 4; i++) if (!ev[i]) CCM_HIP(c, hipEventCreate(&ev[i]));
    CCM_HIP(c, hipEventRecord(ev[0], c->stream));
    int rc = covis_flush(c, d);
    if (rc) return rc;
    // the queries: where each one's hash lies
    const int lds_features = covis_lds_features();
    d->h_q.resize(n_q);
    int lds_cells = 0;
    int64_t g_cells = 0;
    for (int i = 0; i < n_q; i++) {
        const int len = d->entry[q_slot[i]].len, cells = covis_cells(len);
        CovisQ q{ q_slot[i], cells, -1 };
        if (len > lds_features) { q.hash = g_cells; g_cells += cells; } else lds_cells = std::max(lds_cells, cells);
        d->h_q[i] = q;
    }
    if ((rc = ccm_upload(c, d->d_q, d->h_q.data(), (size_t)n_q * sizeof(CovisQ), c->stream))) return rc;
    if (g_cells) CCM_RESERVE(c, d->d_hash, (size_t)g_cells * 8);
    // outputs: one device block [weights | n_mps | n_redundant | skipped]; the download skips the weights nobody asked for
    const size_t w_cells = (size_t)n_q * (size_t)n_slots, out_bytes = (w_cells + 3 * (size_t)n_q) * 4;
    CCM_RESERVE(c, d->d_out, out_bytes);
    const bool want_w = (what & CCM_COVIS_WEIGHTS) != 0;
    const size_t dl_off = want_w ? 0 : w_cells * 4, dl_bytes = out_bytes - dl_off;
    if (dl_bytes > d->h_out_cap) {
        if (d->h_out) (void)hipHostFree(d->h_out);
        d->h_out = nullptr; d->h_out_cap = 0;
        const size_t want = dl_bytes + dl_bytes / 2 + 4096;
        if (hipHostMalloc(&d->h_out, want, hipHostMallocDefault) != hipSuccess) { d->h_out = nullptr; return ccm_fail(c, CCM_E_NOMEM, "%s: %zu bytes of page-locked memory", name, want); }
        d->h_out_cap = want;
    }
    CovisQuery a{};
    a.slots = d->d_slots; a.octave = d->d_octave; a.slot = d->d_slot.as<CovisSlot>(); a.n_slots = n_slots; a.n_q = n_q;
    a.q = d->d_q.as<CovisQ>();
    a.flags = t ? t->T.flags : nullptr; a.flags_capacity = t ? t->capacity : 0;
    a.th_obs = r->th_obs;
    a.g_key = g_cells ? d->d_hash.as<int32_t>() : nullptr; a.g_val = g_cells ? d->d_hash.as<int32_t>() + g_cells : nullptr;
    a.weights = d->d_out.as<int32_t>();
    a.n_mps = a.weights + w_cells; a.n_redundant = a.n_mps + n_q; a.skipped = a.n_redundant + n_q;
    CCM_HIP(c, hipEventRecord(ev[1], c->stream));
    if (g_cells) covis_launch_build(c->stream, a);
    covis_launch_weights(c->stream, a, lds_cells);
    if (what & CCM_COVIS_REDUNDANCY) covis_launch_redundancy(c->stream, a, lds_cells);
    CCM_HIP(c, hipGetLastError());
    CCM_HIP(c, hipEventRecord(ev[2], c->stream));
    CCM_HIP(c, hipMemcpyAsync(d->h_out, d->d_out.as<char>() + dl_off, dl_bytes, hipMemcpyDeviceToHost, c->stream));
    CCM_HIP(c, hipEventRecord(ev[3], c->stream));
    CCM_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t* h = static_cast<const int32_t*>(d->h_out);
    if (want_w) {
        for (int i = 0; i < n_q; i++) std::memcpy(r->weights + (size_t)i * capacity, h + (size_t)i * n_slots, (size_t)n_slots * 4);
        h += w_cells;
    }
    if (r->n_mps) std::memcpy(r->n_mps, h, (size_t)n_q * 4);
    if (what & CCM_COVIS_REDUNDANCY) std::memcpy(r->n_redundant, h + n_q, (size_t)n_q * 4);
    if (r->skipped) std::memcpy(r->skipped, h + 2 * (size_t)n_q, (size_t)n_q * 4);
    if (r->seq) for (int s = 0; s < n_slots; s++) r->seq[s] = d->entry[s].seq;
    for (int i = 0; i < 3; i++) d->last_ms[i] = covis_ms(ev[i], ev[i + 1]);
    return n_slots;
}

int covis_query(ccm_ctx* c, ccm_covis* d, ccm_map_table* t, int n_q, const int64_t* keys, int what, int capacity, ccm_covis_result* r)
{
    const char* name = "ccm_covis_query";
    if (what == 0 || (what & ~(CCM_COVIS_WEIGHTS | CCM_COVIS_REDUNDANCY))) return ccm_fail(c, CCM_E_ARG, "%s: what = %d", name, what);
    if (n_q < 0 || capacity < 0 || (n_q > 0 && (!keys || !r))) return ccm_fail(c, CCM_E_ARG, "%s: null argument", name);
    if (n_q == 0) return CCM_OK;
    if ((what & CCM_COVIS_WEIGHTS) && capacity > 0 && !r->weights) return ccm_fail(c, CCM_E_ARG, "%s: null weights", name);
    if (what & CCM_COVIS_REDUNDANCY) {
        if (!r->n_redundant) return ccm_fail(c, CCM_E_ARG, "%s: null n_redundant", name);
        if (r->th_obs < 1 || r->th_obs > COVIS_MAX_TH_OBS) return ccm_fail(c, CCM_E_ARG, "%s: th_obs %d outside [1, %d]", name, r->th_obs, COVIS_MAX_TH_OBS);
    }
    std::lock_guard<std::mutex> lock(d->mu);
    if (d->device >= 0 && c->device != d->device)
        return ccm_fail(c, CCM_E_ARG, "%s: the context is on device %d, the index on device %d", name, c->device, d->device);
    std::vector<int32_t> q_slot(n_q);
    for (int i = 0; i < n_q; i++) {
        auto it = d->slot_of.find(keys[i]);
        if (it == d->slot_of.end()) return ccm_fail(c, CCM_E_ARG, "%s: key %lld (query %d) is not in the index", name, (long long)keys[i], i);
        q_slot[i] = it->second;
    }
    const int64_t n_slots = (int64_t)d->entry.size();
    if (n_slots > capacity) return ccm_fail(c, CCM_E_CAPACITY, "%s: %lld slots, room for %d", name, (long long)n_slots, capacity);
    if (((n_slots + COVIS_CHUNK - 1) / COVIS_CHUNK) * n_q > 0x7fffffffLL)
        return ccm_fail(c, CCM_E_CAPACITY, "%s: %d queries over %lld slots exceed one launch", name, n_q, (long long)n_slots);
    d->device = c->device;
    const int rc = covis_run(c, d, t, q_slot, what, capacity, r);
    if (rc < 0) (void)hipStreamSynchronize(c->stream);                         // nothing of a failed query stays queued on the staging
    return rc;
}

}  // namespace

extern "C" {

int ccm_covis_create(ccm_ctx* c, int64_t initial_capacity_features, ccm_covis** out)
{
    RoctxRange roctx_("ccm_covis_create");
    return ccm_guard(c, "ccm_covis_create", [&]() -> int {
        if (!out) return CCM_E_ARG;
        *out = nullptr;
        if (initial_capacity_features < 0) return ccm_fail(c, CCM_E_ARG, "ccm_covis_create: initial_capacity_features %lld", (long long)initial_capacity_features);
        std::unique_ptr<ccm_covis> d(new ccm_covis());
        d->initial_cap = initial_capacity_features;
        if (c) {
            CCM_HIP(c, hipSetDevice(c->device));
            d->device = c->device;
            int rc = covis_rebuild(c, d.get(), initial_capacity_features);
            if (rc) { ccm_covis_destroy(d.release()); return rc; }
            d->table_dirty = false;
        }
        *out = d.release();
        return CCM_OK;
    });
}

void ccm_covis_destroy(ccm_covis* d)
{
    if (!d) return;
    if (d->device >= 0) {
        (void)hipSetDevice(d->device);
        if (d->d_slots) (void)hipFree(d->d_slots);
        if (d->d_octave) (void)hipFree(d->d_octave);
        for (hipEvent_t e : d->ev) if (e) (void)hipEventDestroy(e);
        if (d->h_out) (void)hipHostFree(d->h_out);
    }
    delete d;
}

int ccm_covis_put(ccm_covis* d, int64_t key, int n, const int32_t* slot, const uint8_t* octave)
{
    RoctxRange roctx_("ccm_covis_put");
    if (!d || n < 0 || (n > 0 && (!slot || !octave))) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_covis_put", [&]() -> int {
        CovisPending p{ -1, std::vector<int32_t>(slot, slot + n), std::vector<uint8_t>(octave, octave + n) };   // (copied outside the lock)
        std::lock_guard<std::mutex> lock(d->mu);
        d->pending.reserve(d->pending.size() + 1);
        auto it = d->slot_of.find(key);
        if (it != d->slot_of.end()) {                                        // replace: the slot and the sequence number stay
            p.slot = it->second;
            CovisEntry& e = d->entry[p.slot];
            if (e.off < 0) {
                for (CovisPending& q : d->pending)
                    if (q.slot == p.slot) { q = std::move(p); break; }
            } else {
                d->live -= e.len;                                            // its features become a hole in the arena
                e.off = -1;
                d->pending.push_back(std::move(p));
            }
            e.len = n;
            d->table_dirty = true;
            return CCM_OK;
        }
        if (d->free_slots.empty()) { d->entry.emplace_back(); d->free_slots.push_back((int32_t)d->entry.size() - 1); }
        d->slot_of.emplace(key, d->free_slots.back());                       // nothing below throws
        p.slot = d->free_slots.back(); d->free_slots.pop_back();
        CovisEntry& e = d->entry[p.slot];
        e.key = key; e.seq = d->next_seq++; e.off = -1; e.len = n;
        d->pending.push_back(std::move(p));
        d->table_dirty = true;
        return CCM_OK;
    });
}

int ccm_covis_erase(ccm_covis* d, int64_t key)
{
    RoctxRange roctx_("ccm_covis_erase");
    if (!d) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_covis_erase", [&]() -> int {
        std::lock_guard<std::mutex> lock(d->mu);
        auto it = d->slot_of.find(key);
        if (it == d->slot_of.end()) return CCM_OK;                           // nothing to erase
        const int32_t s = it->second;
        d->free_slots.reserve(d->free_slots.size() + 1);
        d->slot_of.erase(it);
        CovisEntry& e = d->entry[s];
        if (e.off < 0) {                                                     // never uploaded: drop it from the pending list
            for (size_t i = 0; i < d->pending.size(); i++)
                if (d->pending[i].slot == s) { d->pending.erase(d->pending.begin() + (long)i); break; }
        } else d->live -= e.len;                                             // its features become a hole in the arena
        e = CovisEntry();
        d->free_slots.push_back(s);
        d->table_dirty = true;
        return CCM_OK;
    });
}

int ccm_covis_clear(ccm_covis* d)
{
    RoctxRange roctx_("ccm_covis_clear");
    if (!d) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_covis_clear", [&]() -> int {
        std::lock_guard<std::mutex> lock(d->mu);
        d->slot_of.clear(); d->entry.clear(); d->free_slots.clear(); d->pending.clear();
        d->used = d->live = 0;
        d->table_dirty = true;
        return CCM_OK;
    });
}

int ccm_covis_size(ccm_covis* d)
{
    if (!d) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    return (int)d->slot_of.size();
}

int ccm_covis_slot(ccm_covis* d, int64_t key)
{
    if (!d) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    auto it = d->slot_of.find(key);
    return it == d->slot_of.end() ? -1 : it->second;
}

int ccm_covis_slots(ccm_covis* d)
{
    if (!d) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    return (int)d->entry.size();
}

int ccm_covis_keys(ccm_covis* d, int capacity, int64_t* keys, int64_t* seq)
{
    if (!d || capacity < 0 || (capacity > 0 && !keys)) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    const int n = (int)d->entry.size();
    if (n > capacity) return CCM_E_CAPACITY;
    for (int s = 0; s < n; s++) { keys[s] = d->entry[s].seq < 0 ? -1 : d->entry[s].key; if (seq) seq[s] = d->entry[s].seq; }
    return n;
}

int ccm_covis_lds_features(void) { return covis_lds_features(); }

int ccm_covis_arena(ccm_covis* d, int64_t* capacity_features, int64_t* used_features, int64_t* live_features)
{
    if (!d) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    if (capacity_features) *capacity_features = d->cap;
    if (used_features) *used_features = d->used;
    if (live_features) *live_features = d->live;
    return CCM_OK;
}

int ccm_covis_last_timing(ccm_covis* d, double ms3[3])
{
    if (!d || !ms3) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    for (int i = 0; i < 3; i++) ms3[i] = d->last_ms[i];
    return CCM_OK;
}

int ccm_covis_query(ccm_ctx* c, ccm_covis* d, ccm_map_table* t, int n_q, const int64_t* query_keys, int what, int capacity, ccm_covis_result* r)
{
    RoctxRange roctx_("ccm_covis_query");
    if (!c) return CCM_E_ARG;
    if (!d) return ccm_fail(c, CCM_E_ARG, "ccm_covis_query: null index");
    if (t) {
        int rc = check_table(c, t);
        if (rc) return rc;
        return table_call(c, t, false, "ccm_covis_query", [&]() -> int { return covis_query(c, d, t, n_q, query_keys, what, capacity, r); });
    }
    return ccm_guard(c, "ccm_covis_query", [&]() -> int { return covis_query(c, d, nullptr, n_q, query_keys, what, capacity, r); });
}

// ---- host step: the ordered lists of UpdateConnections (src/KeyFrame.cpp:664-711)
int ccm_covis_connections(int n_slots, const int32_t* weights, const int32_t* rank, int th, int capacity, int32_t* order_slot, int32_t* order_weight)
{
    RoctxRange roctx_("ccm_covis_connections");
    if (n_slots < 0 || capacity < 0 || (n_slots > 0 && !weights) || (capacity > 0 && !order_slot)) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_covis_connections", [&]() -> int {
        auto before = [&](int32_t a, int32_t b) {                               // a precedes b in the iteration of KFcounter
            if (rank && rank[a] != rank[b]) return rank[a] < rank[b];
            return a < b;
        };
        std::vector<int32_t> listed;
        int32_t best = -1;
        for (int32_t s = 0; s < n_slots; s++) {
            if (weights[s] <= 0) continue;                                      // not in KFcounter
            if (best < 0 || weights[s] > weights[best] || (weights[s] == weights[best] && before(s, best))) best = s;    // :679, strict
            if (weights[s] >= th) listed.push_back(s);                          // :684
        }
        if (best < 0) return 0;                                                 // :664
        if (listed.empty()) listed.push_back(best);                             // :691
        // sort(vPairs) ascending by (weight, position), then push_front: descending by both
        std::sort(listed.begin(), listed.end(), [&](int32_t a, int32_t b) { return weights[a] != weights[b] ? weights[a] > weights[b] : before(b, a); });
        if ((int64_t)listed.size() > capacity) return CCM_E_CAPACITY;
        for (size_t i = 0; i < listed.size(); i++) { order_slot[i] = listed[i]; if (order_weight) order_weight[i] = weights[listed[i]]; }
        return (int)listed.size();
    });
}

}  // extern "C"
