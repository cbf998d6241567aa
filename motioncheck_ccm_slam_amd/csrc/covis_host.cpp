// covis_host.cpp -- C ABI of the device covisibility index (include/ccm_hot.h, section "Covisibility"): the store of one record per
// keyframe (table slot and octave per feature), the batched query that replaces the counter of KeyFrame::UpdateConnections
// (src/KeyFrame.cpp:644-662) and the observer loop of LocalMapping::KeyFrameCullingV3 (src/Mapping.cpp:818-855), and the ordered
// remainder of UpdateConnections replayed on the host over one row of weights (ccm_covis_connections, :664-711).  The store is
// record_store.h, shared with kfdb_host.cpp: host bookkeeping under a mutex, a pending list, an arena that a query grows and compacts.
#include "record_store.h"
#include "mpt_internal.h"
#include "covis_types.h"
#include <cstdlib>
#include <memory>
#include <mutex>

static_assert(COVIS_MP_LIVE == CCM_MP_LIVE && COVIS_MP_BAD == CCM_MP_BAD, "covis_types.h mirrors CCM_MP_*");

namespace {

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

void covis_move(hipStream_t s, const void* const src[2], void* const dst[2], const RecordMoveJob* job, int n_jobs)
{
    covis_launch_move(s, CovisMove{ (const int32_t*)src[0], (const uint8_t*)src[1], (int32_t*)dst[0], (uint8_t*)dst[1], job, n_jobs });
}

}  // namespace

struct ccm_covis {
    std::mutex mu;                          // around every use of `store`; a query holds it from its flush to the end of its download
    RecordStore store{ sizeof(int32_t), sizeof(uint8_t), "ccm_covis_query", "features", covis_move };  // columns: table slots, octaves
    DevBuf d_q, d_hash, d_out;              // d_out: [weights n_q x n_slots | n_mps | n_redundant | skipped]
    std::vector<CovisQ> h_q;                // upload staging: alive until the query's synchronise
};

namespace {

// Under d->mu and, with a table, the shared lock on its rows.  q_slot: the queries' slot numbers, already looked up.
int covis_run(ccm_ctx* c, ccm_covis* d, ccm_map_table* t, const std::vector<int32_t>& q_slot, int what, int capacity, ccm_covis_result* r)
{
    const char* name = "ccm_covis_query";
    RecordStore& st = d->store;
    const int n_q = (int)q_slot.size(), n_slots = st.ix.slots();
    int rc = st.begin(c);
    if (rc == CCM_OK) rc = st.flush(c);
    if (rc) return rc;
    // the queries: where each one's hash lies
    const int lds_features = covis_lds_features();
    d->h_q.resize(n_q);
    int lds_cells = 0;
    int64_t g_cells = 0;
    for (int i = 0; i < n_q; i++) {
        const int len = st.ix.entry[q_slot[i]].len, cells = covis_cells(len);
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
    if ((rc = st.landing(c, name, dl_bytes))) return rc;
    CovisQuery a{};
    a.slots = static_cast<const int32_t*>(st.d_col[0]); a.octave = static_cast<const uint8_t*>(st.d_col[1]);
    a.slot = st.d_slot.as<RecordSlot>(); a.n_slots = n_slots; a.n_q = n_q;
    a.q = d->d_q.as<CovisQ>();
    a.flags = t ? t->T.flags : nullptr; a.flags_capacity = t ? t->capacity : 0;
    a.th_obs = r->th_obs;
    a.g_key = g_cells ? d->d_hash.as<int32_t>() : nullptr; a.g_val = g_cells ? d->d_hash.as<int32_t>() + g_cells : nullptr;
    a.weights = d->d_out.as<int32_t>();
    a.n_mps = a.weights + w_cells; a.n_redundant = a.n_mps + n_q; a.skipped = a.n_redundant + n_q;
    if ((rc = st.mark(c, 1))) return rc;
    if (g_cells) covis_launch_build(c->stream, a);
    covis_launch_weights(c->stream, a, lds_cells);
    if (what & CCM_COVIS_REDUNDANCY) covis_launch_redundancy(c->stream, a, lds_cells);
    CCM_HIP(c, hipGetLastError());
    if ((rc = st.mark(c, 2))) return rc;
    CCM_HIP(c, hipMemcpyAsync(st.h_out, d->d_out.as<char>() + dl_off, dl_bytes, hipMemcpyDeviceToHost, c->stream));
    if ((rc = st.mark(c, 3))) return rc;
    CCM_HIP(c, hipStreamSynchronize(c->stream));
    const int32_t* h = static_cast<const int32_t*>(st.h_out);
    if (want_w) {
        for (int i = 0; i < n_q; i++) std::memcpy(r->weights + (size_t)i * capacity, h + (size_t)i * n_slots, (size_t)n_slots * 4);
        h += w_cells;
    }
    if (r->n_mps) std::memcpy(r->n_mps, h, (size_t)n_q * 4);
    if (what & CCM_COVIS_REDUNDANCY) std::memcpy(r->n_redundant, h + n_q, (size_t)n_q * 4);
    if (r->skipped) std::memcpy(r->skipped, h + 2 * (size_t)n_q, (size_t)n_q * 4);
    if (r->seq) for (int s = 0; s < n_slots; s++) r->seq[s] = st.ix.entry[s].seq;
    st.end();
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
    RecordStore& st = d->store;
    if (st.device >= 0 && c->device != st.device)
        return ccm_fail(c, CCM_E_ARG, "%s: the context is on device %d, the index on device %d", name, c->device, st.device);
    std::vector<int32_t> q_slot(n_q);
    for (int i = 0; i < n_q; i++)
        if ((q_slot[i] = st.ix.find(keys[i])) < 0) return ccm_fail(c, CCM_E_ARG, "%s: key %lld (query %d) is not in the index", name, (long long)keys[i], i);
    const int64_t n_slots = st.ix.slots();
    if (n_slots > capacity) return ccm_fail(c, CCM_E_CAPACITY, "%s: %lld slots, room for %d", name, (long long)n_slots, capacity);
    if (((n_slots + COVIS_CHUNK - 1) / COVIS_CHUNK) * n_q > 0x7fffffffLL)
        return ccm_fail(c, CCM_E_CAPACITY, "%s: %d queries over %lld slots exceed one launch", name, n_q, (long long)n_slots);
    st.device = c->device;                                                     // an index created without a context is bound here
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
        std::unique_ptr<ccm_covis, void (*)(ccm_covis*)> d(new ccm_covis(), ccm_covis_destroy);
        d->store.initial_cap = initial_capacity_features;
        if (c) {                                                             // without a context: bound to the device of the first query
            int rc = d->store.bind(c);
            if (rc) return rc;
        }
        *out = d.release();
        return CCM_OK;
    });
}

void ccm_covis_destroy(ccm_covis* d)
{
    if (!d) return;
    if (d->store.device >= 0) (void)hipSetDevice(d->store.device);
    delete d;
}

int ccm_covis_put(ccm_covis* d, int64_t key, int n, const int32_t* slot, const uint8_t* octave)
{
    RoctxRange roctx_("ccm_covis_put");
    if (!d || n < 0 || (n > 0 && (!slot || !octave))) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_covis_put", [&]() -> int {
        RecordPending p = d->store.ix.stage(n, slot, octave);                 // (copied outside the lock)
        std::lock_guard<std::mutex> lock(d->mu);
        const int32_t s = d->store.ix.find(key);
        if (s >= 0) d->store.ix.replace(s, std::move(p));                    // a keyframe's points change all the time
        else d->store.ix.insert(key, std::move(p));
        return CCM_OK;
    });
}

int ccm_covis_erase(ccm_covis* d, int64_t key)
{
    RoctxRange roctx_("ccm_covis_erase");
    if (!d) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_covis_erase", [&]() -> int { std::lock_guard<std::mutex> lock(d->mu); d->store.ix.erase(key); return CCM_OK; });
}

int ccm_covis_clear(ccm_covis* d)
{
    RoctxRange roctx_("ccm_covis_clear");
    if (!d) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_covis_clear", [&]() -> int { std::lock_guard<std::mutex> lock(d->mu); d->store.ix.clear(); return CCM_OK; });
}

int ccm_covis_size(ccm_covis* d) { if (!d) return CCM_E_ARG; std::lock_guard<std::mutex> lock(d->mu); return d->store.ix.size(); }
int ccm_covis_slot(ccm_covis* d, int64_t key) { if (!d) return CCM_E_ARG; std::lock_guard<std::mutex> lock(d->mu); return d->store.ix.find(key); }
int ccm_covis_slots(ccm_covis* d) { if (!d) return CCM_E_ARG; std::lock_guard<std::mutex> lock(d->mu); return d->store.ix.slots(); }
int ccm_covis_keys(ccm_covis* d, int capacity, int64_t* keys, int64_t* seq) { if (!d) return CCM_E_ARG; std::lock_guard<std::mutex> lock(d->mu); return d->store.keys(capacity, keys, seq); }
int ccm_covis_last_timing(ccm_covis* d, double ms3[3]) { if (!d) return CCM_E_ARG; std::lock_guard<std::mutex> lock(d->mu); return d->store.last_timing(ms3); }

int ccm_covis_lds_features(void) { return covis_lds_features(); }

int ccm_covis_arena(ccm_covis* d, int64_t* capacity_features, int64_t* used_features, int64_t* live_features)
{
    if (!d) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    return d->store.arena(capacity_features, used_features, live_features);
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
