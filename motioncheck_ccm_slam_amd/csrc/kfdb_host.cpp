// kfdb_host.cpp -- C ABI of the device KeyFrameDatabase (include/ccm_hot.h, section "KeyFrameDatabase"): the store behind
// KeyFrameDatabase::add / erase / clear (src/Database.cpp:37-70), the per-entry query that replaces the inverted-file walk of
// DetectLoopCandidates / DetectMapMatchCandidates (:72-327), and the ordered remainder of those two functions replayed on the
// host over the query's arrays (ccm_kfdb_shortlist, ccm_kfdb_candidates), as ccm_sim3_solver_iterate replays Sim3Solver::iterate.
// DetectRelocalizationCandidates (:329-439) is the same shortlist followed by ccm_kfdb_reloc_candidates.
#include "ccm_internal.h"
#include "kfdb_types.h"
#include <cmath>
#include <memory>
#include <mutex>
#include <unordered_map>

namespace {

struct KfdbEntry {                          // one slot, host side
    int64_t key = 0, seq = -1;              // seq < 0: free slot
    int64_t off = -1;                       // place in the arena; -1 while the entry waits in `pending`
    int32_t len = 0;
};

struct KfdbPending { int32_t slot; std::vector<int32_t> ids; std::vector<double> vals; };

int kfdb_check_vector(int n_words, int n, const int32_t* ids, const double* vals)
{
    if (n < 0 || (n > 0 && (!ids || !vals))) return CCM_E_ARG;
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= n_words || (i > 0 && ids[i] <= ids[i - 1])) return CCM_E_ARG;
    return CCM_OK;
}

}  // namespace

struct ccm_kfdb {
    int device = 0, n_words = 0;
    std::mutex mu;
    // ---- host bookkeeping (add / erase / clear touch nothing else)
    std::unordered_map<int64_t, int32_t> slot_of;
    std::vector<KfdbEntry> entry;           // [slots]: its size is the high-water mark
    std::vector<int32_t> free_slots;
    std::vector<KfdbPending> pending;       // added since the last flush, in add order
    int64_t next_seq = 0;
    bool table_dirty = false;               // the device's slot table is behind `entry`
    // ---- device side, touched by queries only (under mu, from the flush to the end of the download)
    int32_t* d_ids = nullptr; double* d_vals = nullptr;
    int64_t cap = 0, used = 0, live = 0;    // arena words: allocated, tail, held by uploaded live entries
    DevBuf d_slot, d_jobs, d_q_ids, d_q_vals, d_out;              // d_out: the query's outputs, [score | words | first_word]
    void* h_out = nullptr; size_t h_out_cap = 0;                  // page-locked landing block of the download
    std::vector<int32_t> h_ids; std::vector<double> h_vals;       // upload staging: alive until the query's synchronise
    std::vector<KfdbSlot> h_slot; std::vector<KfdbMoveJob> h_jobs;
    hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };    // created by the first query
    double last_ms[3] = { 0, 0, 0 };        // flush, kernel, download of the last query (ccm_kfdb_last_timing)
};

namespace {

// Moves the uploaded live entries, packed, into a new arena of new_cap words; the old one is freed once the copy has run.
int kfdb_rebuild(ccm_ctx* c, ccm_kfdb* d, int64_t new_cap)
{
    int32_t* n_ids = nullptr; double* n_vals = nullptr;
    const size_t words = (size_t)std::max<int64_t>(new_cap, 1);
    if (hipMalloc(&n_ids, words * 4) != hipSuccess) return ccm_fail(c, CCM_E_NOMEM, "ccm_kfdb_query: arena of %zu words", words);
    if (hipMalloc(&n_vals, words * 8) != hipSuccess) { (void)hipFree(n_ids); return ccm_fail(c, CCM_E_NOMEM, "ccm_kfdb_query: arena of %zu words", words); }
    d->h_jobs.clear();
    int64_t tail = 0;
    for (KfdbEntry& e : d->entry) {
        if (e.seq < 0 || e.off < 0) continue;
        if (e.len > 0) d->h_jobs.push_back(KfdbMoveJob{ e.off, tail, e.len, 0 });
        e.off = tail; tail += e.len;
    }
    int rc = CCM_OK;
    if (!d->h_jobs.empty()) {
        rc = ccm_upload(c, d->d_jobs, d->h_jobs.data(), d->h_jobs.size() * sizeof(KfdbMoveJob), c->stream);
        if (rc == CCM_OK) {
            kfdb_launch_move(c->stream, KfdbMove{ d->d_ids, d->d_vals, n_ids, n_vals, d->d_jobs.as<KfdbMoveJob>(), (int32_t)d->h_jobs.size() });
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
                rc = ccm_fail(c, CCM_E_DEVICE, "ccm_kfdb_query: moving the arena failed");
        }
    }
    if (d->d_ids) (void)hipFree(d->d_ids);
    if (d->d_vals) (void)hipFree(d->d_vals);
    d->d_ids = n_ids; d->d_vals = n_vals; d->cap = (int64_t)words; d->used = d->live = tail; d->table_dirty = true;
    return rc;
}

// Applies the pending adds and erases: grows or compacts the arena when needed, appends the new entries at its tail and brings
// the device's slot table up to date.  Everything is queued on c->stream.
int kfdb_flush(ccm_ctx* c, ccm_kfdb* d)
{
    int64_t add_words = 0;
    for (const KfdbPending& p : d->pending) add_words += (int64_t)p.ids.size();
    const bool mostly_holes = d->used - d->live > d->used / 2;
    if (mostly_holes || d->used + add_words > d->cap) {
        int64_t new_cap = d->cap;
        if (d->live + add_words > new_cap) new_cap = std::max(2 * d->cap, d->live + add_words);
        int rc = kfdb_rebuild(c, d, new_cap);
        if (rc) return rc;
    }
    if (!d->pending.empty()) {
        d->h_ids.clear(); d->h_vals.clear();
        const int64_t tail = d->used;
        for (const KfdbPending& p : d->pending) {
            KfdbEntry& e = d->entry[p.slot];
            e.off = tail + (int64_t)d->h_ids.size();
            d->h_ids.insert(d->h_ids.end(), p.ids.begin(), p.ids.end());
            d->h_vals.insert(d->h_vals.end(), p.vals.begin(), p.vals.end());
        }
        d->pending.clear();
        d->used += add_words; d->live += add_words; d->table_dirty = true;
        if (add_words) {
            CCM_HIP(c, hipMemcpyAsync(d->d_ids + tail, d->h_ids.data(), (size_t)add_words * 4, hipMemcpyHostToDevice, c->stream));
            CCM_HIP(c, hipMemcpyAsync(d->d_vals + tail, d->h_vals.data(), (size_t)add_words * 8, hipMemcpyHostToDevice, c->stream));
        }
    }
    if (d->table_dirty) {
        d->h_slot.resize(d->entry.size());
        for (size_t s = 0; s < d->entry.size(); s++) {
            const KfdbEntry& e = d->entry[s];
            d->h_slot[s] = e.seq < 0 ? KfdbSlot{ 0, -1, 0 } : KfdbSlot{ e.off, e.len, 0 };
        }
        int rc = ccm_upload(c, d->d_slot, d->h_slot.data(), d->h_slot.size() * sizeof(KfdbSlot), c->stream);
        if (rc) return rc;
        d->table_dirty = false;
    }
    return CCM_OK;
}

double kfdb_ms(hipEvent_t a, hipEvent_t b) { float t = 0; return hipEventElapsedTime(&t, a, b) == hipSuccess ? (double)t : 0.0; }

// stored: the query is the entry of query_key; otherwise it is (n, ids, vals) from the host
int kfdb_query(ccm_ctx* c, ccm_kfdb* d, const char* name, bool stored, int64_t query_key, int n, const int32_t* ids, const double* vals,
               int capacity, int32_t* words, double* score, int32_t* first_word, int64_t* seq)
{
    return ccm_guard(c, name, [&]() -> int {
        if (!c) return CCM_E_ARG;
        if (!d) return ccm_fail(c, CCM_E_ARG, "%s: null database", name);
        if (c->device != d->device) return ccm_fail(c, CCM_E_ARG, "%s: the context is on device %d, the database on device %d", name, c->device, d->device);
        if (capacity < 0 || (capacity > 0 && (!words || !score || !first_word || !seq))) return ccm_fail(c, CCM_E_ARG, "%s: null output array", name);
        if (!stored && kfdb_check_vector(d->n_words, n, ids, vals))
            return ccm_fail(c, CCM_E_ARG, "%s: the query's word ids must be strictly ascending and lie in [0, %d)", name, d->n_words);
        std::lock_guard<std::mutex> lock(d->mu);
        const int n_slots = (int)d->entry.size();
        int32_t q_slot = -1;
        if (stored) {
            auto it = d->slot_of.find(query_key);
            if (it == d->slot_of.end()) return ccm_fail(c, CCM_E_ARG, "%s: key %lld is not in the database", name, (long long)query_key);
            q_slot = it->second;
        }
        if (n_slots > capacity) return ccm_fail(c, CCM_E_CAPACITY, "%s: %d slots, room for %d", name, n_slots, capacity);
        CCM_HIP(c, hipSetDevice(c->device));
        hipEvent_t* ev = d->ev;
        for (int i = 0; i < 4; i++) if (!ev[i]) CCM_HIP(c, hipEventCreate(&ev[i]));
        CCM_HIP(c, hipEventRecord(ev[0], c->stream));
        int rc = kfdb_flush(c, d);
        if (rc) return rc;
        KfdbQuery a{};
        a.ids = d->d_ids; a.vals = d->d_vals; a.slot = d->d_slot.as<KfdbSlot>(); a.n_slots = n_slots;
        if (stored) {
            const KfdbEntry& e = d->entry[q_slot];
            a.q_n = e.len; a.q_ids = d->d_ids + e.off; a.q_vals = d->d_vals + e.off;
        } else {
            if ((rc = ccm_upload(c, d->d_q_ids, ids, (size_t)n * 4, c->stream))) return rc;
            if ((rc = ccm_upload(c, d->d_q_vals, vals, (size_t)n * 8, c->stream))) return rc;
            a.q_n = n; a.q_ids = d->d_q_ids.as<int32_t>(); a.q_vals = d->d_q_vals.as<double>();
        }
        // outputs: one device block [score | words | first_word] and one copy into a page-locked block of the same layout
        const size_t ns = (size_t)n_slots, out_bytes = ns * 16;
        CCM_RESERVE(c, d->d_out, std::max<size_t>(out_bytes, 16));
        if (out_bytes > d->h_out_cap) {
            if (d->h_out) (void)hipHostFree(d->h_out);
            d->h_out = nullptr; d->h_out_cap = 0;
            const size_t want = out_bytes + out_bytes / 2 + 4096;
            if (hipHostMalloc(&d->h_out, want, hipHostMallocDefault) != hipSuccess) { d->h_out = nullptr; return ccm_fail(c, CCM_E_NOMEM, "%s: %zu bytes of page-locked memory", name, want); }
            d->h_out_cap = want;
        }
        a.score = d->d_out.as<double>();
        a.words = reinterpret_cast<int32_t*>(d->d_out.as<char>() + ns * 8);
        a.first_word = reinterpret_cast<int32_t*>(d->d_out.as<char>() + ns * 12);
        CCM_HIP(c, hipEventRecord(ev[1], c->stream));
        kfdb_launch_query(c->stream, a);
        CCM_HIP(c, hipGetLastError());
        CCM_HIP(c, hipEventRecord(ev[2], c->stream));
        if (n_slots) CCM_HIP(c, hipMemcpyAsync(d->h_out, d->d_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
        CCM_HIP(c, hipEventRecord(ev[3], c->stream));
        CCM_HIP(c, hipStreamSynchronize(c->stream));
        if (n_slots) {
            const char* h = static_cast<const char*>(d->h_out);
            std::memcpy(score, h, ns * 8); std::memcpy(words, h + ns * 8, ns * 4); std::memcpy(first_word, h + ns * 12, ns * 4);
        }
        for (int s = 0; s < n_slots; s++) seq[s] = d->entry[s].seq;
        for (int i = 0; i < 3; i++) d->last_ms[i] = kfdb_ms(ev[i], ev[i + 1]);
        return n_slots;
    });
}

}  // namespace

extern "C" {

int ccm_kfdb_create(ccm_ctx* c, int n_words, int64_t initial_capacity_words, ccm_kfdb** out)
{
    RoctxRange roctx_("ccm_kfdb_create");
    return ccm_guard(c, "ccm_kfdb_create", [&]() -> int {
        if (!c || !out) return CCM_E_ARG;
        *out = nullptr;
        if (n_words < 1 || initial_capacity_words < 0) return ccm_fail(c, CCM_E_ARG, "ccm_kfdb_create: n_words %d, initial_capacity_words %lld", n_words, (long long)initial_capacity_words);
        CCM_HIP(c, hipSetDevice(c->device));
        std::unique_ptr<ccm_kfdb> d(new ccm_kfdb());
        d->device = c->device; d->n_words = n_words;
        int rc = kfdb_rebuild(c, d.get(), initial_capacity_words);
        if (rc) { ccm_kfdb_destroy(d.release()); return rc; }
        d->table_dirty = false;
        *out = d.release();
        return CCM_OK;
    });
}

void ccm_kfdb_destroy(ccm_kfdb* d)
{
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->d_ids) (void)hipFree(d->d_ids);
    if (d->d_vals) (void)hipFree(d->d_vals);
    for (hipEvent_t e : d->ev) if (e) (void)hipEventDestroy(e);
    if (d->h_out) (void)hipHostFree(d->h_out);
    delete d;
}

int ccm_kfdb_add(ccm_kfdb* d, int64_t key, int n, const int32_t* ids, const double* vals)
{
    RoctxRange roctx_("ccm_kfdb_add");
    if (!d) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_kfdb_add", [&]() -> int {
        int rc = kfdb_check_vector(d->n_words, n, ids, vals);
        if (rc) return rc;
        KfdbPending p{ -1, std::vector<int32_t>(ids, ids + n), std::vector<double>(vals, vals + n) };      // (copied outside the lock)
        std::lock_guard<std::mutex> lock(d->mu);
        if (d->slot_of.count(key)) return CCM_E_ARG;
        d->pending.reserve(d->pending.size() + 1);
        if (d->free_slots.empty()) { d->entry.emplace_back(); d->free_slots.push_back((int32_t)d->entry.size() - 1); }
        d->slot_of.emplace(key, d->free_slots.back());                       // nothing below throws
        p.slot = d->free_slots.back(); d->free_slots.pop_back();
        KfdbEntry& e = d->entry[p.slot];
        e.key = key; e.seq = d->next_seq++; e.off = -1; e.len = n;
        d->pending.push_back(std::move(p));
        d->table_dirty = true;
        return CCM_OK;
    });
}

int ccm_kfdb_erase(ccm_kfdb* d, int64_t key)
{
    RoctxRange roctx_("ccm_kfdb_erase");
    if (!d) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_kfdb_erase", [&]() -> int {
        std::lock_guard<std::mutex> lock(d->mu);
        auto it = d->slot_of.find(key);
        if (it == d->slot_of.end()) return CCM_OK;                           // as the reference: nothing to erase
        const int32_t s = it->second;
        d->free_slots.reserve(d->free_slots.size() + 1);
        d->slot_of.erase(it);
        KfdbEntry& e = d->entry[s];
        if (e.off < 0) {                                                     // never uploaded: drop it from the pending list
            for (size_t i = 0; i < d->pending.size(); i++)
                if (d->pending[i].slot == s) { d->pending.erase(d->pending.begin() + (long)i); break; }
        } else d->live -= e.len;                                             // its words become a hole in the arena
        e = KfdbEntry();
        d->free_slots.push_back(s);
        d->table_dirty = true;
        return CCM_OK;
    });
}

int ccm_kfdb_clear(ccm_kfdb* d)
{
    RoctxRange roctx_("ccm_kfdb_clear");
    if (!d) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_kfdb_clear", [&]() -> int {
        std::lock_guard<std::mutex> lock(d->mu);
        d->slot_of.clear(); d->entry.clear(); d->free_slots.clear(); d->pending.clear();
        d->used = d->live = 0;
        d->table_dirty = true;
        return CCM_OK;
    });
}

int ccm_kfdb_size(ccm_kfdb* d)
{
    if (!d) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    return (int)d->slot_of.size();
}

int ccm_kfdb_slot(ccm_kfdb* d, int64_t key)
{
    if (!d) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    auto it = d->slot_of.find(key);
    return it == d->slot_of.end() ? -1 : it->second;
}

int ccm_kfdb_slots(ccm_kfdb* d)
{
    if (!d) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    return (int)d->entry.size();
}

int ccm_kfdb_keys(ccm_kfdb* d, int capacity, int64_t* keys, int64_t* seq)
{
    if (!d || capacity < 0 || (capacity > 0 && !keys)) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    const int n = (int)d->entry.size();
    if (n > capacity) return CCM_E_CAPACITY;
    for (int s = 0; s < n; s++) { keys[s] = d->entry[s].seq < 0 ? -1 : d->entry[s].key; if (seq) seq[s] = d->entry[s].seq; }
    return n;
}

int ccm_kfdb_query_lds_words(void) { return KFDB_QUERY_LDS_WORDS; }

int ccm_kfdb_arena(ccm_kfdb* d, int64_t* capacity_words, int64_t* used_words, int64_t* live_words)
{
    if (!d) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    if (capacity_words) *capacity_words = d->cap;
    if (used_words) *used_words = d->used;
    if (live_words) *live_words = d->live;
    return CCM_OK;
}

int ccm_kfdb_last_timing(ccm_kfdb* d, double ms3[3])
{
    if (!d || !ms3) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    for (int i = 0; i < 3; i++) ms3[i] = d->last_ms[i];
    return CCM_OK;
}

int ccm_kfdb_query(ccm_ctx* c, ccm_kfdb* d, int64_t query_key, int capacity, int32_t* words, double* score, int32_t* first_word, int64_t* seq)
{
    RoctxRange roctx_("ccm_kfdb_query");
    return kfdb_query(c, d, "ccm_kfdb_query", true, query_key, 0, nullptr, nullptr, capacity, words, score, first_word, seq);
}

int ccm_kfdb_query_vector(ccm_ctx* c, ccm_kfdb* d, int n, const int32_t* ids, const double* vals, int capacity, int32_t* words,
                          double* score, int32_t* first_word, int64_t* seq)
{
    RoctxRange roctx_("ccm_kfdb_query_vector");
    return kfdb_query(c, d, "ccm_kfdb_query_vector", false, 0, n, ids, vals, capacity, words, score, first_word, seq);
}

// ---- host steps: the ordered remainder of DetectLoopCandidates / DetectMapMatchCandidates (src/Database.cpp:111-201, :236-326)

static inline bool kfdb_listed(int s, const int32_t* words, const int64_t* seq, const uint8_t* eligible, int query_slot)
{
    return seq[s] >= 0 && s != query_slot && eligible[s] && words[s] > 0;
}

int ccm_kfdb_shortlist(int n_slots, const int32_t* words, const double* score, const int32_t* first_word, const int64_t* seq,
                       const uint8_t* eligible, int query_slot, float min_score, int capacity, int32_t* shortlist, int32_t* min_common_words)
{
    RoctxRange roctx_("ccm_kfdb_shortlist");
    if (n_slots < 0 || capacity < 0 || !min_common_words || (n_slots > 0 && (!words || !score || !first_word || !seq || !eligible))) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_kfdb_shortlist", [&]() -> int {
        *min_common_words = 0;
        // lKFsSharingWords: the walk meets an entry first at its smallest common word, and within a word's list in add order
        std::vector<int32_t> listed;
        int max_common = 0;
        for (int s = 0; s < n_slots; s++)
            if (kfdb_listed(s, words, seq, eligible, query_slot)) { listed.push_back(s); max_common = std::max(max_common, words[s]); }
        if (listed.empty()) return 0;
        std::sort(listed.begin(), listed.end(), [&](int32_t a, int32_t b) {
            return first_word[a] != first_word[b] ? first_word[a] < first_word[b] : seq[a] < seq[b]; });
        const int min_common = (int)(max_common * 0.8f);                        // :124
        int n = 0;
        for (int32_t s : listed) {
            if (!(words[s] > min_common)) continue;
            const float si = (float)score[s];
            if (!(si >= min_score)) continue;
            if (n >= capacity || !shortlist) return CCM_E_CAPACITY;
            shortlist[n++] = s;
        }
        if (n) *min_common_words = min_common;
        return n;
    });
}

int ccm_kfdb_candidates(int n_slots, const int32_t* words, const double* score, const int64_t* seq, const uint8_t* eligible, int query_slot,
                        float min_score, int min_common_words, int n_shortlist, const int32_t* shortlist, const int32_t* neighbours,
                        int32_t* candidates)
{
    RoctxRange roctx_("ccm_kfdb_candidates");
    if (n_slots < 0 || n_shortlist < 0 || (n_shortlist > 0 && (!words || !score || !seq || !eligible || !shortlist || !neighbours || !candidates))) return CCM_E_ARG;
    for (int i = 0; i < n_shortlist; i++) if (shortlist[i] < 0 || shortlist[i] >= n_slots) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_kfdb_candidates", [&]() -> int {
        std::vector<float> acc(n_shortlist);
        std::vector<int32_t> best_kf(n_shortlist);
        float best_acc = min_score;                                             // :149
        for (int i = 0; i < n_shortlist; i++) {
            const int32_t s = shortlist[i];
            float best = (float)score[s], a = best;
            int32_t kf = s;
            for (int k = 0; k < CCM_KFDB_NEIGHBOURS; k++) {
                const int32_t nb = neighbours[(size_t)i * CCM_KFDB_NEIGHBOURS + k];
                if (nb < 0 || nb >= n_slots) continue;
                if (!kfdb_listed(nb, words, seq, eligible, query_slot) || !(words[nb] > min_common_words)) continue;      // :164
                const float sn = (float)score[nb];
                a += sn;
                if (sn > best) { kf = nb; best = sn; }
            }
            acc[i] = a; best_kf[i] = kf;
            if (a > best_acc) best_acc = a;
        }
        const float retain = 0.75f * best_acc;                                  // :181
        int n = 0;
        for (int i = 0; i < n_shortlist; i++) {
            if (!(acc[i] > retain)) continue;
            bool seen = false;
            for (int j = 0; j < n && !seen; j++) seen = candidates[j] == best_kf[i];
            if (!seen) candidates[n++] = best_kf[i];
        }
        return n;
    });
}

// The covisibility accumulation of DetectRelocalizationCandidates (src/Database.cpp:372-436) behind ccm_kfdb_shortlist.  mRelocScore is
// the caller's reloc_score: a neighbour that shares a word with the query (mRelocQuery == F.mId, :403) counts whether this query
// scored it or not, with whatever the array holds for it.
int ccm_kfdb_reloc_candidates(int n_slots, const int32_t* words, const double* score, const int64_t* seq, int n_shortlist,
                              const int32_t* shortlist, const int32_t* neighbours, float* reloc_score, int32_t* candidates)
{
    RoctxRange roctx_("ccm_kfdb_reloc_candidates");
    if (n_slots < 0 || n_shortlist < 0 || (n_shortlist > 0 && (!words || !score || !seq || !shortlist || !neighbours || !reloc_score || !candidates)))
        return CCM_E_ARG;
    for (int i = 0; i < n_shortlist; i++) if (shortlist[i] < 0 || shortlist[i] >= n_slots) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_kfdb_reloc_candidates", [&]() -> int {
        for (int i = 0; i < n_shortlist; i++) reloc_score[shortlist[i]] = (float)score[shortlist[i]];       // :379-380, all before :392
        std::vector<float> acc(n_shortlist);
        std::vector<int32_t> best_kf(n_shortlist);
        float best_acc = 0;                                                     // :389
        for (int i = 0; i < n_shortlist; i++) {
            const int32_t s = shortlist[i];
            float best = (float)score[s], a = best;                             // it->first
            int32_t kf = s;
            for (int k = 0; k < CCM_KFDB_NEIGHBOURS; k++) {
                const int32_t nb = neighbours[(size_t)i * CCM_KFDB_NEIGHBOURS + k];
                if (nb < 0 || nb >= n_slots) continue;
                if (seq[nb] < 0 || !(words[nb] > 0)) continue;                  // :403
                const float sn = reloc_score[nb];
                a += sn;
                if (sn > best) { kf = nb; best = sn; }
            }
            acc[i] = a; best_kf[i] = kf;
            if (a > best_acc) best_acc = a;
        }
        const float retain = 0.75f * best_acc;                                  // :420
        int n = 0;
        for (int i = 0; i < n_shortlist; i++) {
            if (!(acc[i] > retain)) continue;
            bool seen = false;
            for (int j = 0; j < n && !seen; j++) seen = candidates[j] == best_kf[i];
            if (!seen) candidates[n++] = best_kf[i];
        }
        return n;
    });
}

float ccm_kfdb_min_score(int n_slots, const double* score, const int64_t* seq, int n_connected, const int32_t* connected)
{
    float min_score = 1;                                                        // LoopFinder.cpp:127, MapMatcher.cpp:135
    if (!score || !seq || !connected) return min_score;
    for (int i = 0; i < n_connected; i++) {
        const int32_t s = connected[i];
        if (s < 0 || s >= n_slots || seq[s] < 0) continue;
        const float si = (float)score[s];
        if (si < min_score) min_score = si;
    }
    return min_score;
}

}  // extern "C"
