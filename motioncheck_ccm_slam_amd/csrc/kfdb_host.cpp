// kfdb_host.cpp -- C ABI of the device KeyFrameDatabase (include/ccm_hot.h, section "KeyFrameDatabase"): the store behind
// KeyFrameDatabase::add / erase / clear (src/Database.cpp:37-70), the per-entry query that replaces the inverted-file walk of
// DetectLoopCandidates / DetectMapMatchCandidates (:72-327), and the ordered remainder of those two functions replayed on the
// host over the query's arrays (ccm_kfdb_shortlist, ccm_kfdb_candidates), as ccm_sim3_solver_iterate replays Sim3Solver::iterate.
// DetectRelocalizationCandidates (:329-439) is the same shortlist followed by ccm_kfdb_reloc_candidates.
// The store itself is record_store.h, shared with covis_host.cpp; what is kept here is the check of the word ids and the query.
#include "record_store.h"
#include "kfdb_types.h"
#include <cmath>
#include <memory>
#include <mutex>

namespace {

int kfdb_check_vector(int n_words, int n, const int32_t* ids, const double* vals)
{
    if (n < 0 || (n > 0 && (!ids || !vals))) return CCM_E_ARG;
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= n_words || (i > 0 && ids[i] <= ids[i - 1])) return CCM_E_ARG;
    return CCM_OK;
}

void kfdb_move(hipStream_t s, const void* const src[2], void* const dst[2], const RecordMoveJob* job, int n_jobs)
{
    kfdb_launch_move(s, KfdbMove{ (const int32_t*)src[0], (const double*)src[1], (int32_t*)dst[0], (double*)dst[1], job, n_jobs });
}

}  // namespace

struct ccm_kfdb {
    int n_words = 0;
    std::mutex mu;                          // around every use of `store`; a query holds it from its flush to the end of its download
    RecordStore store{ sizeof(int32_t), sizeof(double), "ccm_kfdb_query", "words", kfdb_move };       // columns: ids, values
    DevBuf d_q_ids, d_q_vals, d_out;        // d_out: the query's outputs, [score | words | first_word]
};

namespace {

// stored: the query is the entry of query_key; otherwise it is (n, ids, vals) from the host
int kfdb_query(ccm_ctx* c, ccm_kfdb* d, const char* name, bool stored, int64_t query_key, int n, const int32_t* ids, const double* vals,
               int capacity, int32_t* words, double* score, int32_t* first_word, int64_t* seq)
{
    return ccm_guard(c, name, [&]() -> int {
        if (!c) return CCM_E_ARG;
        if (!d) return ccm_fail(c, CCM_E_ARG, "%s: null database", name);
        RecordStore& st = d->store;
        if (c->device != st.device) return ccm_fail(c, CCM_E_ARG, "%s: the context is on device %d, the database on device %d", name, c->device, st.device);
        if (capacity < 0 || (capacity > 0 && (!words || !score || !first_word || !seq))) return ccm_fail(c, CCM_E_ARG, "%s: null output array", name);
        if (!stored && kfdb_check_vector(d->n_words, n, ids, vals))
            return ccm_fail(c, CCM_E_ARG, "%s: the query's word ids must be strictly ascending and lie in [0, %d)", name, d->n_words);
        std::lock_guard<std::mutex> lock(d->mu);
        const int n_slots = st.ix.slots();
        const int32_t q_slot = stored ? st.ix.find(query_key) : -1;
        if (stored && q_slot < 0) return ccm_fail(c, CCM_E_ARG, "%s: key %lld is not in the database", name, (long long)query_key);
        if (n_slots > capacity) return ccm_fail(c, CCM_E_CAPACITY, "%s: %d slots, room for %d", name, n_slots, capacity);
        int rc = st.begin(c);
        if (rc == CCM_OK) rc = st.flush(c);
        if (rc) return rc;
        KfdbQuery a{};
        a.ids = static_cast<const int32_t*>(st.d_col[0]); a.vals = static_cast<const double*>(st.d_col[1]);
        a.slot = st.d_slot.as<RecordSlot>(); a.n_slots = n_slots;
        if (stored) {
            const RecordEntry& e = st.ix.entry[q_slot];
            a.q_n = e.len; a.q_ids = a.ids + e.off; a.q_vals = a.vals + e.off;
        } else {
            if ((rc = ccm_upload(c, d->d_q_ids, ids, (size_t)n * 4, c->stream))) return rc;
            if ((rc = ccm_upload(c, d->d_q_vals, vals, (size_t)n * 8, c->stream))) return rc;
            a.q_n = n; a.q_ids = d->d_q_ids.as<int32_t>(); a.q_vals = d->d_q_vals.as<double>();
        }
        // outputs: one device block [score | words | first_word] and one copy into a page-locked block of the same layout
        const size_t ns = (size_t)n_slots, out_bytes = ns * 16;
        CCM_RESERVE(c, d->d_out, std::max<size_t>(out_bytes, 16));
        if ((rc = st.landing(c, name, out_bytes))) return rc;
        a.score = d->d_out.as<double>();
        a.words = reinterpret_cast<int32_t*>(d->d_out.as<char>() + ns * 8);
        a.first_word = reinterpret_cast<int32_t*>(d->d_out.as<char>() + ns * 12);
        if ((rc = st.mark(c, 1))) return rc;
        kfdb_launch_query(c->stream, a);
        CCM_HIP(c, hipGetLastError());
        if ((rc = st.mark(c, 2))) return rc;
        if (n_slots) CCM_HIP(c, hipMemcpyAsync(st.h_out, d->d_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
        if ((rc = st.mark(c, 3))) return rc;
        CCM_HIP(c, hipStreamSynchronize(c->stream));
        if (n_slots) {
            const char* h = static_cast<const char*>(st.h_out);
            std::memcpy(score, h, ns * 8); std::memcpy(words, h + ns * 8, ns * 4); std::memcpy(first_word, h + ns * 12, ns * 4);
        }
        for (int s = 0; s < n_slots; s++) seq[s] = st.ix.entry[s].seq;
        st.end();
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
        std::unique_ptr<ccm_kfdb, void (*)(ccm_kfdb*)> d(new ccm_kfdb(), ccm_kfdb_destroy);
        d->n_words = n_words; d->store.initial_cap = initial_capacity_words;
        int rc = d->store.bind(c);
        if (rc) return rc;
        *out = d.release();
        return CCM_OK;
    });
}

void ccm_kfdb_destroy(ccm_kfdb* d)
{
    if (!d) return;
    if (d->store.device >= 0) (void)hipSetDevice(d->store.device);
    delete d;
}

int ccm_kfdb_add(ccm_kfdb* d, int64_t key, int n, const int32_t* ids, const double* vals)
{
    RoctxRange roctx_("ccm_kfdb_add");
    if (!d) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_kfdb_add", [&]() -> int {
        int rc = kfdb_check_vector(d->n_words, n, ids, vals);
        if (rc) return rc;
        RecordPending p = d->store.ix.stage(n, ids, vals);                    // (copied outside the lock)
        std::lock_guard<std::mutex> lock(d->mu);
        if (d->store.ix.find(key) >= 0) return CCM_E_ARG;
        d->store.ix.insert(key, std::move(p));
        return CCM_OK;
    });
}

int ccm_kfdb_erase(ccm_kfdb* d, int64_t key)
{
    RoctxRange roctx_("ccm_kfdb_erase");
    if (!d) return CCM_E_ARG;                                                // (an absent key, as the reference: nothing to erase)
    return ccm_guard(nullptr, "ccm_kfdb_erase", [&]() -> int { std::lock_guard<std::mutex> lock(d->mu); d->store.ix.erase(key); return CCM_OK; });
}

int ccm_kfdb_clear(ccm_kfdb* d)
{
    RoctxRange roctx_("ccm_kfdb_clear");
    if (!d) return CCM_E_ARG;
    return ccm_guard(nullptr, "ccm_kfdb_clear", [&]() -> int { std::lock_guard<std::mutex> lock(d->mu); d->store.ix.clear(); return CCM_OK; });
}

int ccm_kfdb_size(ccm_kfdb* d) { if (!d) return CCM_E_ARG; std::lock_guard<std::mutex> lock(d->mu); return d->store.ix.size(); }
int ccm_kfdb_slot(ccm_kfdb* d, int64_t key) { if (!d) return CCM_E_ARG; std::lock_guard<std::mutex> lock(d->mu); return d->store.ix.find(key); }
int ccm_kfdb_slots(ccm_kfdb* d) { if (!d) return CCM_E_ARG; std::lock_guard<std::mutex> lock(d->mu); return d->store.ix.slots(); }
int ccm_kfdb_keys(ccm_kfdb* d, int capacity, int64_t* keys, int64_t* seq) { if (!d) return CCM_E_ARG; std::lock_guard<std::mutex> lock(d->mu); return d->store.keys(capacity, keys, seq); }
int ccm_kfdb_last_timing(ccm_kfdb* d, double ms3[3]) { if (!d) return CCM_E_ARG; std::lock_guard<std::mutex> lock(d->mu); return d->store.last_timing(ms3); }

int ccm_kfdb_query_lds_words(void) { return KFDB_QUERY_LDS_WORDS; }

int ccm_kfdb_arena(ccm_kfdb* d, int64_t* capacity_words, int64_t* used_words, int64_t* live_words)
{
    if (!d) return CCM_E_ARG;
    std::lock_guard<std::mutex> lock(d->mu);
    return d->store.arena(capacity_words, used_words, live_words);
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
