// cslam_covisibility.cpp -- the covisibility index of include/ccm_hot.h ("Covisibility") behind the two host walks of the server
// that count shared map points: the counter of cslam::KeyFrame::UpdateConnections (src/KeyFrame.cpp:633-662) and the loop of
// cslam::LocalMapping::KeyFrameCullingV3 (src/Mapping.cpp:804-862).
//
// Unlike the other shim files this one defines no member function of the reference.  Both functions keep their own walk in their own
// file, because the walk is the fallback: the calls below return false whenever the index cannot answer (the process is not the
// server, the library has no context on this thread, a keyframe has no record or a point of it has no table slot yet), and the
// reference's text then runs as it stands.  INTEGRATION.md ("Covisibility index") shows the two places where they are called:
//
//   KeyFrame::UpdateConnections   std::map<kfptr,int> KFcounter;
//                                 if (!ccm_shim::covis_counter(shared_from_this(), mSysState == eSystemState::SERVER, KFcounter))
//                                     { ... the reference's loop :635-662 ... }
//                                 ... the reference's text from :664 on, unchanged: KFcounter is the same std::map, so its iteration
//                                 order, the threshold, the ordered lists and the parent selection are the reference's own
//   LocalMapping::KeyFrameCullingV3   in front of the loop :804:
//                                 if (ccm_shim::covis_cull(vpLocalKeyFrames, protect, params::mapping::mfRedundancyThres, mCulledKfs)) return;
//                                 with protect(pKF) = the tests of :807 and :810
//   KeyFrame::SetBadFlag          ccm_shim::covis_dropped(mId) beside ccm_shim::keyframe_dropped
//
//   wherever ccm_shim::keyframe_touched(id) is called (the hooks keyframe_handle uses: AddMapPoint, EraseMapPointMatch,
//   ReplaceMapPointMatch, ...)   ccm_shim::covis_touched(shared_from_this()) beside it
//
// Every count runs against every stored keyframe, so every keyframe's record has to be current, not only the querying one's.
// covis_touched only notes the keyframe (it may be called under the keyframe's own mutex); the next call below builds the records of
// the noted keyframes again, each one only when its stamp is not the one its record was built at.  One index serves the whole
// process: keyframes of different maps share no point, so they weigh 0 for each other.
#include <cslam/KeyFrame.h>
#include <cslam/MapPoint.h>
#include <boost/weak_ptr.hpp>
#include <climits>
#include <functional>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>
#include "ccm_shim.h"
#include "fuse_steps.h"

namespace ccm_shim {

typedef boost::shared_ptr<cslam::KeyFrame> covis_kfptr;

namespace {

struct CovisRecord {
    boost::weak_ptr<cslam::KeyFrame> kf;
    uint64_t stamp = 0;                 // the keyframe's stamp the record was built at; 0 = build it again
    bool all_slotted = false;           // every map point of it had a table slot
};

struct CovisSide {
    std::mutex m;                       // guards `of`; the index has its own mutex
    ccm_covis* index = nullptr;
    std::unordered_map<int64_t, CovisRecord> of;
    std::vector<int64_t> touched;       // keyframes a hook noted since the last flush
    ~CovisSide() { ccm_covis_destroy(index); }
};

CovisSide& covis_side()
{
    static CovisSide s;
    return s;
}

// (id, client) of a keyframe as one key: ids stay below 2^40, client numbers below 2^23 (as the KeyFrameDatabase's keys)
inline int64_t covis_key(const cslam::idpair& id) { return (int64_t)(((uint64_t)id.second << 40) | (uint64_t)id.first); }

ccm_covis* covis_index()
{
    CovisSide& S = covis_side();
    std::lock_guard<std::mutex> lock(S.m);
    if (!S.index && ccm_covis_create(nullptr, (int64_t)1 << 22, &S.index)) S.index = nullptr;     // bound to the first querying context's device
    return S.index;
}

// The record of pKF is current in the index; false when a point of it has no table slot (the index cannot speak for it)
bool covis_sync(ccm_covis* index, const covis_kfptr& pKF)
{
    CovisSide& S = covis_side();
    const int64_t key = covis_key(pKF->mId);
    const uint64_t now = keyframe_stamp(pKF->mId.first, pKF->mId.second);
    {
        std::lock_guard<std::mutex> lock(S.m);
        const auto it = S.of.find(key);
        if (it != S.of.end() && now != 0 && it->second.stamp == now) return it->second.all_slotted;
    }
    const std::vector<boost::shared_ptr<cslam::MapPoint>> vpMP = pKF->GetMapPointMatches();
    const int n = (int)vpMP.size();
    std::vector<int32_t> slot(n);
    std::vector<uint8_t> octave(n);
    bool all_slotted = true;
    for (int i = 0; i < n; i++) {
        const int s = vpMP[i] ? map_slot_of(vpMP[i]) : -1;
        slot[i] = !vpMP[i] ? -1 : s >= 0 ? s : INT32_MAX;
        if (vpMP[i] && s < 0) all_slotted = false;
        const int o = pKF->mvKeysUn[i].octave;
        octave[i] = (uint8_t)(o < 0 ? 0 : o > 255 ? 255 : o);
    }
    if (ccm_covis_put(index, key, n, slot.data(), octave.data())) return false;
    std::lock_guard<std::mutex> lock(S.m);
    CovisRecord& r = S.of[key];
    r.kf = pKF; r.stamp = all_slotted ? now : 0; r.all_slotted = all_slotted;      // (no stamp kept: built again once the slots exist)
    return all_slotted;
}

// The records of the keyframes the hooks noted are built again
void covis_flush_touched(ccm_covis* index)
{
    CovisSide& S = covis_side();
    std::vector<covis_kfptr> kfs;
    {
        std::lock_guard<std::mutex> lock(S.m);
        for (int64_t key : S.touched) {
            const auto it = S.of.find(key);
            if (it == S.of.end()) continue;
            if (covis_kfptr kf = it->second.kf.lock()) kfs.push_back(kf);
        }
        S.touched.clear();
    }
    for (const covis_kfptr& kf : kfs)
        if (!kf->isBad()) covis_sync(index, kf);
}

struct CovisRows {
    int n_slots = 0;
    std::vector<int32_t> weights, n_mps, n_redundant, skipped;
    std::vector<int64_t> seq, key;
};

bool covis_query(ccm_covis* index, const std::vector<int64_t>& keys, int what, CovisRows& R)
{
    ccm_map_table* table = map_table_here();
    if (!ctx() || !table) return false;
    const int n_q = (int)keys.size();
    for (;;) {
        const int cap = ccm_covis_slots(index) + 256;                              // room for the puts of other threads
        if (what & CCM_COVIS_WEIGHTS) R.weights.resize((size_t)n_q * cap);
        R.n_mps.resize(n_q); R.n_redundant.resize(n_q); R.skipped.resize(n_q); R.seq.resize(cap); R.key.resize(cap);
        ccm_covis_result res{3, R.weights.data(), R.n_mps.data(), R.n_redundant.data(), R.skipped.data(), R.seq.data()};
        const int rc = ccm_covis_query(ctx(), index, table, n_q, keys.data(), what, cap, &res);
        if (rc == CCM_E_CAPACITY) continue;
        if (rc < 0) return false;
        R.n_slots = rc;
        // the keys as of now; a slot that changed hands since the query is told apart by its sequence number
        std::vector<int64_t> seq_now(cap);
        const int m = ccm_covis_keys(index, cap, R.key.data(), seq_now.data());
        for (int s = 0; s < R.n_slots; s++)
            if (s >= m || seq_now[s] != R.seq[s]) R.key[s] = -1;
        return true;
    }
}

}  // namespace

// The hooks that call keyframe_touched: the keyframe's map points changed.  Cheap, and safe under the keyframe's own mutexes.
void covis_touched(const covis_kfptr& pKF)
{
    if (!pKF) return;
    CovisSide& S = covis_side();
    std::lock_guard<std::mutex> lock(S.m);
    const int64_t key = covis_key(pKF->mId);
    S.of[key].kf = pKF;
    S.touched.push_back(key);
}

// KeyFrame::SetBadFlag: the keyframe leaves the index (pKFi->isBad() of src/Mapping.cpp:835 is "not stored")
void covis_dropped(const cslam::idpair& id)
{
    CovisSide& S = covis_side();
    ccm_covis* index;
    {
        std::lock_guard<std::mutex> lock(S.m);
        S.of.erase(covis_key(id));
        index = S.index;
    }
    if (index) ccm_covis_erase(index, covis_key(id));
}

// KFcounter of KeyFrame::UpdateConnections (src/KeyFrame.cpp:633-662) for pKF from the index.  false: KFcounter is untouched and the
// caller walks the observations itself.
bool covis_counter(const covis_kfptr& pKF, bool is_server, std::map<covis_kfptr, int>& KFcounter)
{
    if (!is_server || !pKF || pKF->isBad()) return false;
    ccm_covis* index = covis_index();
    if (!index) return false;
    covis_flush_touched(index);
    if (!covis_sync(index, pKF)) return false;
    CovisRows R;
    const int64_t key = covis_key(pKF->mId);
    if (!covis_query(index, std::vector<int64_t>(1, key), CCM_COVIS_WEIGHTS, R)) return false;
    std::map<covis_kfptr, int> counter;
    CovisSide& S = covis_side();
    std::vector<std::pair<int64_t, int>> hits;
    for (int s = 0; s < R.n_slots; s++)
        if (R.weights[s] > 0) { if (R.key[s] < 0) return false; hits.push_back(std::make_pair(R.key[s], R.weights[s])); }
    {
        std::lock_guard<std::mutex> lock(S.m);
        for (const auto& h : hits) {
            const auto it = S.of.find(h.first);
            const covis_kfptr other = it == S.of.end() ? covis_kfptr() : it->second.kf.lock();
            if (!other) return false;                                           // a stored keyframe nobody holds any more: walk the map
            counter[other] = h.second;
        }
    }
    KFcounter.swap(counter);
    return true;
}

// The loop of LocalMapping::KeyFrameCullingV3 (src/Mapping.cpp:804-862) over vpLocalKeyFrames: one query for all of them, the verdict
// of :857 in double, and at the first keyframe that is culled SetBadFlag, the index without it, and a new query for the keyframes
// behind it (SetBadFlag takes its observations away, and points left with two observers turn bad: the map-point table learns of them
// through the hooks of MapPoint::SetBadFlag before the next query reads it).  false: nothing was done, the caller runs its own loop.
bool covis_cull(const std::vector<covis_kfptr>& vpLocalKeyFrames, const std::function<bool(const covis_kfptr&)>& protect,
                double redundancy_thres, int& n_culled)
{
    ccm_covis* index = covis_index();
    if (!index) return false;
    std::vector<covis_kfptr> todo;
    for (const covis_kfptr& pKF : vpLocalKeyFrames)
        if (pKF && !protect(pKF)) todo.push_back(pKF);
    covis_flush_touched(index);
    for (const covis_kfptr& pKF : todo)
        if (pKF->isBad() || !covis_sync(index, pKF)) return false;
    bool any = false;
    while (!todo.empty()) {
        std::vector<int64_t> keys;
        for (const covis_kfptr& pKF : todo) keys.push_back(covis_key(pKF->mId));
        CovisRows R;
        if (!covis_query(index, keys, CCM_COVIS_REDUNDANCY, R)) return any;      // (after a cull the rest of the list is left for the next call)
        size_t i = 0;
        for (; i < todo.size(); i++)
            if ((double)R.n_redundant[i] > redundancy_thres * (double)R.n_mps[i]) break;
        if (i == todo.size()) break;
        const covis_kfptr pKF = todo[i];
        pKF->SetBadFlag();                                                      // calls covis_dropped through its hook
        covis_dropped(pKF->mId);                                                // (and here, should the hook be missing)
        ++n_culled;
        any = true;
        todo.erase(todo.begin(), todo.begin() + (long)i + 1);
        covis_flush_touched(index);                                             // points that turned bad left their keyframes
        for (const covis_kfptr& rest : todo)
            if (rest->isBad() || !covis_sync(index, rest)) return true;
    }
    return true;
}

}  // namespace ccm_shim
