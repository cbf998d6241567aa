// ccm_shim.h -- shared by the three drop-in translation units of this directory.
//
// These files REPLACE cslam/src/ORBextractor.cpp, the hot entry points of cslam/src/ORBmatcher.cpp and the bundle-adjustment
// entry points of src/Optimizer.cpp in a CCM-SLAM checkout: same classes, same signatures (the reference's own headers
// include/cslam/{ORBextractor,ORBmatcher,Optimizer}.h stay untouched), bodies forward to the C ABI of libccm_hot.so
// (include/ccm_hot.h).  They need the reference's headers and its dependencies (OpenCV, Boost, ROS messages), so they are
// compiled by shim/CMakeLists.txt only where find_package(OpenCV) succeeds and CCM_SLAM_INCLUDE_DIR points at a checkout;
// in this repository tests/test_shim_cpu.py checks every ccm_* call in them against the prototypes of ccm_hot.h.
#pragma once
#include <ccm_hot.h>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace ccm_shim {

// One context (HIP stream + workspaces) per calling thread: Tracking, LocalMapping, LoopFinder and MapMatcher each run in
// their own thread in the reference (src/ClientHandler.cpp:140-176), and a ccm_ctx is not meant to be shared.  The same
// thread-local object caches the device-resident frames (ccm_frame) of the two Frames Tracking works on -- the current one and
// mLastFrame -- so that the Frame-side SearchByProjection bodies upload a Frame's keypoints and descriptors once, not per call.
// Members are destroyed in reverse order: the frames go before the context.
struct ThreadState {
    struct Slot { size_t id0 = ~(size_t)0, id1 = ~(size_t)0; int n = -1; ccm_frame* f = nullptr; unsigned used = 0; };
    // a shim object built against another version of ccm_hot.h than the library would pass structures of the wrong size
    ccm_ctx* c = ccm_abi_version() == CCM_ABI_VERSION ? ccm_create(0, 0) : nullptr;
    ccm_vocabulary* voc = nullptr;                     // this thread's copy of the vocabulary (vocabulary() below)
    Slot slot[2];
    unsigned clock = 0;
    ThreadState() = default;
    ThreadState(const ThreadState&) = delete;
    ThreadState& operator=(const ThreadState&) = delete;
    ~ThreadState()
    {
        for (Slot& s : slot) ccm_frame_destroy(s.f);
        ccm_voc_destroy(voc);
        if (c) ccm_destroy(c);
    }
};
inline ThreadState& thread_state()
{
    static thread_local ThreadState s;
    return s;
}
inline ccm_ctx* ctx()
{
    return thread_state().c;                           // nullptr: every ccm_* call returns CCM_E_ARG and the shim bodies throw
}

// ---- the vocabulary.  A ccm_vocabulary lives on one context's device, so every thread that transforms (Tracking: Frame::ComputeBoW
// on the frame handle) makes its own from the node arrays registered once after ORBVocabulary::loadFromTextFile (INTEGRATION.md
// "ORBVocabulary": parent, descriptor and weight of m_nodes[i], with m_k, m_L, m_weighting, m_scoring).
struct VocabularyArrays {
    std::mutex m;
    int k = 0, L = 0, weighting = 0, scoring = 0;
    std::vector<int32_t> parent; std::vector<uint8_t> desc; std::vector<double> weight;
};
inline VocabularyArrays& vocabulary_arrays()
{
    static VocabularyArrays v;
    return v;
}
// This thread's vocabulary, made on first use; nullptr when none is registered or it cannot be created
inline ccm_vocabulary* vocabulary()
{
    ThreadState& S = thread_state();
    if (S.voc) return S.voc;
    VocabularyArrays& V = vocabulary_arrays();
    std::lock_guard<std::mutex> lock(V.m);
    if (V.parent.empty()) return nullptr;
    if (ccm_voc_create(S.c, V.k, V.L, (int)V.parent.size(), V.parent.data(), V.desc.data(), V.weight.data(), &S.voc)) S.voc = nullptr;
    return S.voc;
}

// CCM_SHIM_FRAME_HANDLES=0: the Frame-side matchers go back to uploading the Frame per call (A/B timing of the two paths)
inline bool frame_handles_on()
{
    static const bool on = !(getenv("CCM_SHIM_FRAME_HANDLES") && atoi(getenv("CCM_SHIM_FRAME_HANDLES")) == 0);
    return on;
}

#ifdef FRAME_GRID_COLS                                 // translation units that include cslam/Frame.h
// The cached ccm_frame of Frame F, keyed on Frame::mId and checked against N (a Frame's mvKeysUn and mDescriptors never change after
// its constructor), made on a miss in the least recently used slot; nullptr on failure.
template <class FrameT>
inline ccm_frame* frame_handle(const FrameT& F)
{
    ThreadState& S = thread_state();
    const int N = (int)F.mvKeysUn.size();
    S.clock++;
    for (ThreadState::Slot& s : S.slot)
        if (s.f && s.id0 == F.mId.first && s.id1 == F.mId.second && s.n == N) { s.used = S.clock; return s.f; }
    ThreadState::Slot& s = S.slot[0].used <= S.slot[1].used ? S.slot[0] : S.slot[1];
    ccm_frame_destroy(s.f);
    s = ThreadState::Slot();
    std::vector<float> kx(N), ky(N), angle(N); std::vector<int32_t> oct(N);
    for (int i = 0; i < N; i++) { kx[i] = F.mvKeysUn[i].pt.x; ky[i] = F.mvKeysUn[i].pt.y; oct[i] = F.mvKeysUn[i].octave; angle[i] = F.mvKeysUn[i].angle; }
    const auto desc = F.mDescriptors.isContinuous() ? F.mDescriptors : F.mDescriptors.clone();
    const ccm_frame_grid g{N, kx.data(), ky.data(), oct.data(), desc.data, FrameT::mnMinX, FrameT::mnMinY, FrameT::mfGridElementWidthInv,
                           FrameT::mfGridElementHeightInv, FRAME_GRID_COLS, FRAME_GRID_ROWS};
    ccm_frame* f = nullptr;
    if (ccm_frame_create(S.c, &g, angle.data(), &f)) return nullptr;
    s.id0 = F.mId.first; s.id1 = F.mId.second; s.n = N; s.f = f; s.used = S.clock;
    return f;
}
// A handle made elsewhere for Frame F (the constructor's device route, cslam_frame.cpp: ccm_frame_from_extract_camera) goes into the
// least recently used slot, so that frame_handle(F) finds it and nothing of F is uploaded.  The cache owns f from here on.
template <class FrameT>
inline void frame_handle_put(const FrameT& F, ccm_frame* f)
{
    ThreadState& S = thread_state();
    S.clock++;
    ThreadState::Slot& s = S.slot[0].used <= S.slot[1].used ? S.slot[0] : S.slot[1];
    ccm_frame_destroy(s.f);
    s = ThreadState::Slot();
    s.id0 = F.mId.first; s.id1 = F.mId.second; s.n = ccm_frame_size(f); s.f = f; s.used = S.clock;
}
#endif

// ---- keyframe handles (cslam_mapping.cpp).  LocalMapping keeps one ccm_frame per keyframe of its neighbourhood in ITS context (a
// handle belongs to the context that made it; LoopFinder and MapMatcher run in other threads and must not use it).  A keyframe's
// features never change; its map-point matches and its pose do, from any thread.  The hooks below are called by the reference where
// that happens (INTEGRATION.md "Keyframe handles": KeyFrame::AddMapPoint, EraseMapPointMatch, ReplaceMapPointMatch, SetPose call
// keyframe_touched; KeyFrame::SetBadFlag calls keyframe_dropped); the cache sends mp_id and the pose again when the stamp it saw is
// not the current one.  A keyframe no hook has ever touched has no stamp and is sent again on every use: forgetting the hooks costs
// 8 KB per keyframe and call, never a stale match.  Memory: the cache holds at most kMaxKeyframeHandles handles (least recently used
// go first, about 250 KB of device memory each at 2000 features); the stamp table holds one entry per live keyframe.
struct KeyframeStamps {
    std::mutex m;
    std::map<std::pair<size_t, size_t>, uint64_t> stamp;       // absent = never touched; one entry per live keyframe a hook touched
    std::vector<std::pair<size_t, size_t>> dropped;            // SetBadFlag since LocalMapping last looked; drained by its cache
};
inline KeyframeStamps& keyframe_stamps()
{
    static KeyframeStamps s;
    return s;
}
inline void keyframe_touched(size_t id0, size_t id1)
{
    KeyframeStamps& S = keyframe_stamps();
    std::lock_guard<std::mutex> lock(S.m);
    S.stamp[std::make_pair(id0, id1)]++;
}
// The stamp goes and the id is queued for the cache, which destroys the handle when LocalMapping next enters one of its two calls.
inline void keyframe_dropped(size_t id0, size_t id1)
{
    KeyframeStamps& S = keyframe_stamps();
    std::lock_guard<std::mutex> lock(S.m);
    S.stamp.erase(std::make_pair(id0, id1));
    S.dropped.push_back(std::make_pair(id0, id1));
}
// 0 = never touched
inline uint64_t keyframe_stamp(size_t id0, size_t id1)
{
    KeyframeStamps& S = keyframe_stamps();
    std::lock_guard<std::mutex> lock(S.m);
    const auto it = S.stamp.find(std::make_pair(id0, id1));
    return it == S.stamp.end() ? 0 : it->second;
}
// The keyframes dropped since the last call (the list is emptied)
inline std::vector<std::pair<size_t, size_t>> keyframes_dropped()
{
    KeyframeStamps& S = keyframe_stamps();
    std::lock_guard<std::mutex> lock(S.m);
    std::vector<std::pair<size_t, size_t>> out;
    out.swap(S.dropped);
    return out;
}
static const size_t kMaxKeyframeHandles = 192;    // SearchInNeighbors names up to 20 + 20 * 5 keyframes in one call
// CCM_SHIM_KEYFRAME_HANDLES=0: CreateNewMapPoints and SearchInNeighbors go back to uploading every keyframe per call
inline bool keyframe_handles_on()
{
    static const bool on = !(getenv("CCM_SHIM_KEYFRAME_HANDLES") && atoi(getenv("CCM_SHIM_KEYFRAME_HANDLES")) == 0);
    return on;
}

// per-feature vocabulary node of a DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>), -1 = none
template <class FeatVec>
inline std::vector<int32_t> nodes_of(const FeatVec& fv, int n)
{
    std::vector<int32_t> node(n, -1);
    for (const auto& kv : fv)
        for (unsigned i : kv.second) if ((int)i < n) node[i] = (int32_t)kv.first;
    return node;
}

}  // namespace ccm_shim
