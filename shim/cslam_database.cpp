// cslam_database.cpp -- drop-in bodies of cslam::KeyFrameDatabase::add / erase / clear / DetectLoopCandidates /
// DetectMapMatchCandidates / DetectRelocalizationCandidates (src/Database.cpp:37-439) on the device KeyFrameDatabase of
// include/ccm_hot.h.  The constructor and the map-point bookkeeping stay the reference's: remove the six bodies above from
// src/Database.cpp and link this file.  The reference's header (include/cslam/Database.h) stays untouched, so the
// ccm_kfdb handle and the key -> keyframe table live in a side table keyed on the object; mvInvertedFile stays empty.
//
// What the walk read from the keyframes while it ran is handed over as arrays: `eligible` from the map's keyframes and
// GetConnectedKeyFrames() (loop) or from msuAssClients (map match), the neighbours of each shortlisted keyframe from
// GetBestCovisibilityKeyFrames(10).  ccm_shim::kfdb_min_score below is the minScore loop of LoopFinder.cpp:122-139 /
// MapMatcher.cpp:130-147 from the scores of the same kind of query, without a second pass over the BowVectors.
#include <cslam/Database.h>
#include <cslam/KeyFrame.h>
#include <cslam/Map.h>
#include <cmath>
#include <map>
#include <mutex>
#include <stdexcept>
#include <unordered_map>
#include "ccm_shim.h"

namespace ccm_shim {

typedef boost::shared_ptr<cslam::KeyFrame> kfdb_kfptr;

struct KfdbSide {
    ccm_kfdb* db = nullptr;
    std::unordered_map<int64_t, kfdb_kfptr> kf;            // what is stored, by key
    std::vector<float> reloc_score;                        // mRelocScore per slot (ccm_kfdb_reloc_candidates), 0 from add on
    ~KfdbSide() { ccm_kfdb_destroy(db); }
};

static std::mutex g_kfdb_mutex;                            // guards the side table and every KfdbSide::kf
static std::map<const void*, KfdbSide>& kfdb_table()
{
    static std::map<const void*, KfdbSide> t;
    return t;
}

// (id, client) of a keyframe as one key: ids stay below 2^40, client numbers below 2^23
static inline int64_t kfdb_key(const idpair& id) { return (int64_t)(((uint64_t)id.second << 40) | (uint64_t)id.first); }

// The side entry of a database object, with its device database made on first use (n_words = the vocabulary's size)
static KfdbSide& kfdb_side(const void* self, int n_words)
{
    KfdbSide& S = kfdb_table()[self];
    if (!S.db && ccm_kfdb_create(ctx(), n_words, (int64_t)1 << 22, &S.db)) throw std::runtime_error(ccm_last_error(ctx()));
    return S;
}

struct KfdbQueryArrays {
    int n = 0, query_slot = -1;
    std::vector<int32_t> words, first_word;
    std::vector<double> score;
    std::vector<int64_t> seq, key;
};

// ccm_kfdb_query for a stored keyframe, with the key of every slot; the arrays are sized with room for the adds of other threads
static void kfdb_query(ccm_kfdb* db, int64_t key, KfdbQueryArrays& A)
{
    for (;;) {
        const int cap = ccm_kfdb_slots(db) + 256;
        A.words.resize(cap); A.first_word.resize(cap); A.score.resize(cap); A.seq.resize(cap); A.key.resize(cap);
        const int rc = ccm_kfdb_query(ctx(), db, key, cap, A.words.data(), A.score.data(), A.first_word.data(), A.seq.data());
        if (rc == CCM_E_CAPACITY) continue;
        if (rc < 0) throw std::runtime_error(ccm_last_error(ctx()));
        A.n = rc;
        break;
    }
    // the keys as of now; a slot that changed hands since the query is told apart by its sequence number
    std::vector<int64_t> seq_now(A.key.size());
    const int m = ccm_kfdb_keys(db, (int)A.key.size(), A.key.data(), seq_now.data());
    for (int s = 0; s < A.n; s++)
        if (s >= m || seq_now[s] != A.seq[s]) A.key[s] = -1;
    A.query_slot = ccm_kfdb_slot(db, key);
}

// Host steps A and B over one query; eligible has A.n bytes
static std::vector<kfdb_kfptr> kfdb_detect(KfdbSide& S, const KfdbQueryArrays& A, const std::vector<uint8_t>& eligible, float minScore)
{
    std::vector<kfdb_kfptr> out;
    std::vector<int32_t> shortlist(A.n > 0 ? A.n : 1);
    int32_t min_common = 0;
    const int n_short = ccm_kfdb_shortlist(A.n, A.words.data(), A.score.data(), A.first_word.data(), A.seq.data(), eligible.data(), A.query_slot, minScore,
                                           (int)shortlist.size(), shortlist.data(), &min_common);
    if (n_short <= 0) return out;
    std::vector<int32_t> neighbours((size_t)n_short * CCM_KFDB_NEIGHBOURS, -1), candidates(n_short);
    std::vector<kfdb_kfptr> kf_of_slot(A.n);
    {
        std::lock_guard<std::mutex> lock(g_kfdb_mutex);
        for (int s = 0; s < A.n; s++) {
            const auto it = A.key[s] < 0 ? S.kf.end() : S.kf.find(A.key[s]);
            if (it != S.kf.end()) kf_of_slot[s] = it->second;
        }
    }
    for (int i = 0; i < n_short; i++) {
        const kfdb_kfptr& pKFi = kf_of_slot[shortlist[i]];
        if (!pKFi) continue;
        const std::vector<kfdb_kfptr> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
        for (size_t k = 0; k < vpNeighs.size() && k < CCM_KFDB_NEIGHBOURS; k++) {
            const int32_t s = ccm_kfdb_slot(S.db, kfdb_key(vpNeighs[k]->mId));
            neighbours[(size_t)i * CCM_KFDB_NEIGHBOURS + k] = (s >= 0 && s < A.n && kf_of_slot[s] == vpNeighs[k]) ? s : -1;
        }
    }
    const int n_cand = ccm_kfdb_candidates(A.n, A.words.data(), A.score.data(), A.seq.data(), eligible.data(), A.query_slot, minScore, min_common, n_short,
                                           shortlist.data(), neighbours.data(), candidates.data());
    for (int i = 0; i < n_cand; i++)
        if (kf_of_slot[candidates[i]]) out.push_back(kf_of_slot[candidates[i]]);
    return out;
}

// minScore of LoopFinder.cpp:122-139 / MapMatcher.cpp:130-147: float 1 lowered to the least score of the connected keyframes that
// are not bad and are stored.  One query; DetectLoopCandidates / DetectMapMatchCandidates run their own afterwards.
float kfdb_min_score(cslam::KeyFrameDatabase* self, const kfdb_kfptr& pKF, const std::vector<kfdb_kfptr>& vpConnectedKeyFrames)
{
    ccm_kfdb* db;
    {
        std::lock_guard<std::mutex> lock(g_kfdb_mutex);
        const auto it = kfdb_table().find(self);
        if (it == kfdb_table().end() || !it->second.db) return 1.0f;
        db = it->second.db;
    }
    KfdbQueryArrays A;
    kfdb_query(db, kfdb_key(pKF->mId), A);
    std::vector<int32_t> connected;
    for (const kfdb_kfptr& k : vpConnectedKeyFrames)
        if (!k->isBad()) connected.push_back(ccm_kfdb_slot(db, kfdb_key(k->mId)));
    return ccm_kfdb_min_score(A.n, A.score.data(), A.seq.data(), (int)connected.size(), connected.data());
}

}  // namespace ccm_shim

namespace cslam {

using namespace ccm_shim;

void KeyFrameDatabase::add(kfptr pKF)
{
    std::vector<int32_t> ids; std::vector<double> vals;
    for (DBoW2::BowVector::const_iterator vit = pKF->mBowVec.begin(); vit != pKF->mBowVec.end(); vit++) {      // a std::map: key order
        ids.push_back((int32_t)vit->first); vals.push_back(vit->second);
    }
    std::lock_guard<std::mutex> lock(g_kfdb_mutex);
    KfdbSide& S = kfdb_side(this, (int)mpVoc->size());
    const int64_t key = kfdb_key(pKF->mId);
    if (ccm_kfdb_add(S.db, key, (int)ids.size(), ids.data(), vals.data()) == CCM_OK) {
        S.kf[key] = pKF;
        const int slot = ccm_kfdb_slot(S.db, key);          // a new keyframe, also in a slot another one held: mRelocScore starts at 0
        if (slot >= (int)S.reloc_score.size()) S.reloc_score.resize((size_t)slot + 1, 0.0f);
        if (slot >= 0) S.reloc_score[slot] = 0.0f;
    }
}

void KeyFrameDatabase::erase(kfptr pKF)
{
    std::lock_guard<std::mutex> lock(g_kfdb_mutex);
    KfdbSide& S = kfdb_side(this, (int)mpVoc->size());
    const int64_t key = kfdb_key(pKF->mId);
    ccm_kfdb_erase(S.db, key);
    S.kf.erase(key);
}

void KeyFrameDatabase::clear()
{
    std::lock_guard<std::mutex> lock(g_kfdb_mutex);
    KfdbSide& S = kfdb_side(this, (int)mpVoc->size());
    ccm_kfdb_clear(S.db);
    S.kf.clear();
    S.reloc_score.clear();
}

vector<KeyFrameDatabase::kfptr> KeyFrameDatabase::DetectLoopCandidates(kfptr pKF, float minScore)
{
    const set<kfptr> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
    const std::map<idpair, kfptr> mpAllKfsInMap = pKF->GetMapptr()->GetMmpKeyFrames();
    KfdbSide* S;
    {
        std::lock_guard<std::mutex> lock(g_kfdb_mutex);
        S = &kfdb_side(this, (int)mpVoc->size());
    }
    KfdbQueryArrays A;
    kfdb_query(S->db, kfdb_key(pKF->mId), A);
    // eligible: in the query's map, not connected to it (the query's own slot is left out by the host step)
    std::vector<uint8_t> eligible(A.n > 0 ? A.n : 1, 0);
    for (std::map<idpair, kfptr>::const_iterator mit = mpAllKfsInMap.begin(); mit != mpAllKfsInMap.end(); mit++) {
        const int s = ccm_kfdb_slot(S->db, kfdb_key(mit->first));
        if (s >= 0 && s < A.n && A.key[s] == kfdb_key(mit->first) && !spConnectedKeyFrames.count(mit->second)) eligible[s] = 1;
    }
    return kfdb_detect(*S, A, eligible, minScore);
}

vector<KeyFrameDatabase::kfptr> KeyFrameDatabase::DetectMapMatchCandidates(kfptr pKF, float minScore, mapptr pMap)
{
    KfdbSide* S;
    {
        std::lock_guard<std::mutex> lock(g_kfdb_mutex);
        S = &kfdb_side(this, (int)mpVoc->size());
    }
    KfdbQueryArrays A;
    kfdb_query(S->db, kfdb_key(pKF->mId), A);
    // eligible: the entry's client (the upper part of its key) is not associated with the query's map
    std::vector<uint8_t> eligible(A.n > 0 ? A.n : 1, 0);
    for (int s = 0; s < A.n; s++)
        if (A.key[s] >= 0 && !pMap->msuAssClients.count((size_t)((uint64_t)A.key[s] >> 40))) eligible[s] = 1;
    return kfdb_detect(*S, A, eligible, minScore);
}

// :329-439: the query vector is the frame's, every stored entry is eligible and there is no minimum score; the accumulation reads and
// writes the per-slot mRelocScore kept beside the database (ccm_kfdb_reloc_candidates).
vector<KeyFrameDatabase::kfptr> KeyFrameDatabase::DetectRelocalizationCandidates(Frame& F)
{
    std::vector<int32_t> ids; std::vector<double> vals;
    for (DBoW2::BowVector::const_iterator vit = F.mBowVec.begin(); vit != F.mBowVec.end(); vit++) {
        ids.push_back((int32_t)vit->first); vals.push_back(vit->second);
    }
    KfdbSide* S;
    {
        std::lock_guard<std::mutex> lock(g_kfdb_mutex);
        S = &kfdb_side(this, (int)mpVoc->size());
    }
    KfdbQueryArrays A;
    for (;;) {
        const int cap = ccm_kfdb_slots(S->db) + 256;
        A.words.resize(cap); A.first_word.resize(cap); A.score.resize(cap); A.seq.resize(cap); A.key.resize(cap);
        const int rc = ccm_kfdb_query_vector(ctx(), S->db, (int)ids.size(), ids.data(), vals.data(), cap, A.words.data(), A.score.data(),
                                             A.first_word.data(), A.seq.data());
        if (rc == CCM_E_CAPACITY) continue;
        if (rc < 0) throw std::runtime_error(ccm_last_error(ctx()));
        A.n = rc;
        break;
    }
    std::vector<int64_t> seq_now(A.key.size());
    const int m = ccm_kfdb_keys(S->db, (int)A.key.size(), A.key.data(), seq_now.data());
    for (int s = 0; s < A.n; s++)
        if (s >= m || seq_now[s] != A.seq[s]) A.key[s] = -1;
    vector<kfptr> out;
    const std::vector<uint8_t> eligible(A.n > 0 ? A.n : 1, 1);
    std::vector<int32_t> shortlist(A.n > 0 ? A.n : 1);
    int32_t min_common = 0;
    const int n_short = ccm_kfdb_shortlist(A.n, A.words.data(), A.score.data(), A.first_word.data(), A.seq.data(), eligible.data(), -1, -INFINITY,
                                           (int)shortlist.size(), shortlist.data(), &min_common);
    if (n_short <= 0) return out;
    std::vector<int32_t> neighbours((size_t)n_short * CCM_KFDB_NEIGHBOURS, -1), candidates(n_short);
    std::vector<kfptr> kf_of_slot(A.n);
    {
        std::lock_guard<std::mutex> lock(g_kfdb_mutex);
        for (int s = 0; s < A.n; s++) {
            const auto it = A.key[s] < 0 ? S->kf.end() : S->kf.find(A.key[s]);
            if (it != S->kf.end()) kf_of_slot[s] = it->second;
        }
    }
    for (int i = 0; i < n_short; i++) {                    // outside the lock, as kfdb_detect: the keyframes take their own mutexes
        const kfptr& pKFi = kf_of_slot[shortlist[i]];
        if (!pKFi) continue;
        const std::vector<kfptr> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
        for (size_t k = 0; k < vpNeighs.size() && k < CCM_KFDB_NEIGHBOURS; k++) {
            const int32_t s = ccm_kfdb_slot(S->db, kfdb_key(vpNeighs[k]->mId));
            neighbours[(size_t)i * CCM_KFDB_NEIGHBOURS + k] = (s >= 0 && s < A.n && kf_of_slot[s] == vpNeighs[k]) ? s : -1;
        }
    }
    int n_cand;
    {
        std::lock_guard<std::mutex> lock(g_kfdb_mutex);    // the score array is the side table's; add resizes and zeroes it
        if ((int)S->reloc_score.size() < A.n) S->reloc_score.resize(A.n, 0.0f);
        n_cand = ccm_kfdb_reloc_candidates(A.n, A.words.data(), A.score.data(), A.seq.data(), n_short, shortlist.data(), neighbours.data(),
                                           S->reloc_score.data(), candidates.data());
    }
    for (int i = 0; i < n_cand; i++)
        if (kf_of_slot[candidates[i]]) out.push_back(kf_of_slot[candidates[i]]);
    return out;
}

}  // namespace cslam
