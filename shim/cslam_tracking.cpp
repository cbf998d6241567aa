// cslam_tracking.cpp -- drop-in bodies of cslam::Tracking::SearchLocalPoints (src/Tracking.cpp:860-922) and
// Tracking::TrackLocalMap (:623-727) on the device-resident map-point table (ccm_hot.h "map-point table").  The reference visits
// every map point of the client's map on every tracked image (this fork sets mvpLocalMapPoints = mpMap->GetAllMapPoints(), :924-934)
// and calls Frame::isInFrustum on each; here the map lives in a ccm_map_table, ONE ccm_frame_search_local_points call does both loops
// and the matcher, and ONE ccm_frame_pose_optimize_table call the pose.  Remove these two bodies from src/Tracking.cpp; the rest of
// the file stays as it is.
//
// The table is filled where the map changes, not here: INTEGRATION.md "Map-point table" lists the one-line hooks in Map::AddMapPoint
// / EraseMapPoint and MapPoint::SetWorldPos / UpdateNormalAndDepth / ComputeDistinctiveDescriptors / SetBadFlag that call
// ccm_shim::MapTable::put / erase below.  The hooks sit inside MapPoint because the raw mfMinDistance / mfMaxDistance are private
// (GetMinDistanceInvariance returns 0.8f * mfMinDistance, which cannot be divided back exactly).
#include <cslam/Tracking.h>
#include <cslam/Frame.h>
#include <cslam/MapPoint.h>
#include <cslam/Map.h>
#include <cslam/Optimizer.h>
#include <cslam/Converter.h>
#include <map>
#include <mutex>
#include "ccm_shim.h"

namespace ccm_shim {

// The slot map of one client's map: slot <-> map point, filled where map points are created and erased.  Slots are handed out in
// creation order and reused after an erase.  The visiting order of SearchLocalPoints is the order of Map::mmpMapPoints (a std::map
// keyed by idpair, src/Map.cpp:416-424); it is sent again only when the set of points has changed.  One table per tracking thread:
// the hooks run in other threads (LocalMapping, Communicator), so they only queue rows under the mutex, and the tracking thread
// sends them with ccm_map_table_update before it searches.
class MapTable {
public:
    using mpptr = cslam::Tracking::mpptr;
    static MapTable& get()
    {
        static MapTable t;
        return t;
    }
    // Map::AddMapPoint and every MapPoint setter: queue the row of pMP (all columns).  min_dist / max_dist are the raw members.
    void put(const mpptr& pMP, float min_dist, float max_dist)
    {
        std::lock_guard<std::mutex> lock(mMutex);
        auto it = mSlotOf.find(pMP->mId);
        int slot;
        if (it != mSlotOf.end()) slot = it->second;
        else {
            if (!mFree.empty()) { slot = mFree.back(); mFree.pop_back(); }
            else { slot = (int)mPoints.size(); mPoints.push_back(nullptr); mRows.push_back(Row{}); }
            mSlotOf[pMP->mId] = slot; mPoints[slot] = pMP; mOrderDirty = true;
        }
        Row r;
        r.slot = slot;
        const cv::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal(), D = pMP->GetDescriptor();
        for (int k = 0; k < 3; k++) { r.pos[k] = P.empty() ? 0.f : P.at<float>(k); r.normal[k] = Pn.empty() ? 0.f : Pn.at<float>(k); }
        r.min_dist = min_dist; r.max_dist = max_dist;
        for (int k = 0; k < 32; k++) r.desc[k] = D.empty() ? 0 : D.at<uint8_t>(0, k);
        r.flags = CCM_MP_LIVE | (pMP->isBad() ? CCM_MP_BAD : 0) | (pMP->Observations() > 0 ? CCM_MP_HAS_OBS : 0);
        mQueue.push_back(r);
        mRows[slot] = r;
    }
    // Map::EraseMapPoint: the slot is free again
    void erase(const mpptr& pMP)
    {
        std::lock_guard<std::mutex> lock(mMutex);
        auto it = mSlotOf.find(pMP->mId);
        if (it == mSlotOf.end()) return;
        Row r{};
        r.slot = it->second; r.flags = 0;
        mQueue.push_back(r);
        mRows[it->second] = r;
        mPoints[it->second] = nullptr; mFree.push_back(it->second); mSlotOf.erase(it); mOrderDirty = true;
    }
    int slot_of(const mpptr& pMP)
    {
        std::lock_guard<std::mutex> lock(mMutex);
        auto it = mSlotOf.find(pMP->mId);
        return it == mSlotOf.end() ? -1 : it->second;
    }
    mpptr point(int slot)
    {
        std::lock_guard<std::mutex> lock(mMutex);
        return slot >= 0 && slot < (int)mPoints.size() ? mPoints[slot] : nullptr;
    }
    // The tracking thread, before it searches: the queued rows and, when the set of points changed, the order.  Returns the table.
    ccm_map_table* flush()
    {
        std::lock_guard<std::mutex> lock(mMutex);
        ccm_ctx* c = ctx();
        const int need = (int)mPoints.size();
        if (!mTable || ccm_map_table_capacity(mTable) < need) {                // grow: a new table, the last row of every live slot again
            ccm_map_table* bigger = nullptr;
            if (ccm_map_table_create(c, std::max(2 * need, 65536), &bigger)) return nullptr;
            ccm_map_table_destroy(mTable);
            mTable = bigger; mOrderDirty = true;
            std::vector<Row> all;
            for (int s = 0; s < need; s++) if (mPoints[s]) all.push_back(mRows[s]);     // bad points that still own a slot included
            all.insert(all.end(), mQueue.begin(), mQueue.end());                         // rows queued by other threads stay behind them
            mQueue.swap(all);
        }
        const int n = (int)mQueue.size();
        if (n > 0) {
            std::vector<int32_t> slot(n); std::vector<float> pos(3 * (size_t)n), normal(3 * (size_t)n), mn(n), mx(n);
            std::vector<uint8_t> desc(32 * (size_t)n), flags(n);
            for (int i = 0; i < n; i++) {
                const Row& r = mQueue[i];
                slot[i] = r.slot; mn[i] = r.min_dist; mx[i] = r.max_dist; flags[i] = r.flags;
                for (int k = 0; k < 3; k++) { pos[3 * (size_t)i + k] = r.pos[k]; normal[3 * (size_t)i + k] = r.normal[k]; }
                for (int k = 0; k < 32; k++) desc[32 * (size_t)i + k] = r.desc[k];
            }
            const ccm_map_update u{n, slot.data(), pos.data(), normal.data(), mn.data(), mx.data(), desc.data(), flags.data()};
            if (ccm_map_table_update(c, mTable, &u)) return nullptr;
            mQueue.clear();
        }
        if (mOrderDirty) {
            std::vector<int32_t> order;
            order.reserve(mSlotOf.size());
            for (const auto& kv : mSlotOf) order.push_back(kv.second);         // ascending idpair, as mmpMapPoints
            if (ccm_map_table_set_order(c, mTable, (int)order.size(), order.empty() ? &mZero : order.data())) return nullptr;
            mOrderDirty = false;
        }
        return mTable;
    }
    // The slots in view of the previous SearchLocalPoints: Frame::isInFrustum clears mbTrackInView of every point it tests, so a
    // point that was in view and is rejected now must not keep a stale `true`.
    std::vector<int32_t> mLastInView;

private:
    struct Row { int slot; float pos[3], normal[3], min_dist, max_dist; uint8_t desc[32]; uint8_t flags; };
    std::mutex mMutex;
    std::map<cslam::idpair, int> mSlotOf;
    std::vector<mpptr> mPoints;
    std::vector<int> mFree;
    std::vector<Row> mQueue, mRows;                       // mRows: the last row sent for a slot, with the raw distances
    ccm_map_table* mTable = nullptr;
    bool mOrderDirty = true;
    int32_t mZero = 0;
};

}  // namespace ccm_shim

namespace cslam {

namespace {

// mvpMapPoints of the current frame as slots into the handle
bool send_frame_points(ccm_frame* h, const Frame& F)
{
    std::vector<int32_t> ids(std::max(F.N, 1), -1);
    ccm_shim::MapTable& T = ccm_shim::MapTable::get();
    for (int i = 0; i < F.N; i++) if (F.mvpMapPoints[i]) ids[i] = T.slot_of(F.mvpMapPoints[i]);
    return ccm_frame_set_map_points(h, ids.data()) == 0;
}

}  // namespace

void Tracking::SearchLocalPoints()
{
    ccm_shim::MapTable& T = ccm_shim::MapTable::get();
    ccm_map_table* table = T.flush();
    Frame& F = *mCurrentFrame;
    ccm_frame* h = ccm_shim::frame_handle(F);
    if (!table || !h || !send_frame_points(h, F)) throw estd::infrastructure_ex();

    ccm_slp_params p{};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) p.Tcw[4 * r + c] = F.mTcw.at<float>(r, c);
        p.Tcw[4 * r + 3] = F.mTcw.at<float>(r, 3);
    }
    const cv::Mat Ow = F.GetCameraCenter();
    for (int k = 0; k < 3; k++) p.Ow[k] = Ow.at<float>(k);
    p.fx = Frame::fx; p.fy = Frame::fy; p.cx = Frame::cx; p.cy = Frame::cy;
    p.min_x = Frame::mnMinX; p.max_x = Frame::mnMaxX; p.min_y = Frame::mnMinY; p.max_y = Frame::mnMaxY;
    p.viewing_cos_limit = 0.5f;                                                // :902
    p.log_scale_factor = F.mfLogScaleFactor; p.n_levels = F.mnScaleLevels; p.scale_factors = F.mvScaleFactors.data();
    p.th = mCurrentFrame->mId.first < mLastRelocFrameId.first + 2 ? 5.f : 1.f; // :913-918
    p.nnratio = 0.8f;                                                          // :912

    const int cap = ccm_map_table_capacity(table);
    std::vector<int32_t> in_view(cap), match(std::max(F.N, 1)), ids(std::max(F.N, 1));
    std::vector<float> px(cap), py(cap), vc(cap);
    std::vector<int32_t> level(cap);
    ccm_slp_result r{0, cap, in_view.data(), px.data(), py.data(), level.data(), vc.data(), match.data(), ids.data(), nullptr};
    if (ccm_frame_search_local_points(ccm_shim::ctx(), h, table, &p, &r) < 0) throw estd::infrastructure_ex();

    // the side effects of :863-879 on the frame's own points, from the returned ids (bad ones cleared) ...
    for (int i = 0; i < F.N; i++) {
        mpptr& pMP = F.mvpMapPoints[i];
        if (!pMP) continue;
        if (ids[i] < 0 || (match[i] >= 0 && pMP->isBad())) pMP = nullptr;      // :868-871 (a cleared feature may have been matched anew)
        else { pMP->IncreaseVisible(); pMP->mLastFrameSeen = F.mId; pMP->mbTrackInView = false; }
    }
    // ... of :902-906 on the points in view (the fields isInFrustum leaves on them) ...
    for (int32_t s : T.mLastInView) if (mpptr pMP = T.point(s)) pMP->mbTrackInView = false;       // src/Frame.cpp:141
    T.mLastInView.assign(in_view.begin(), in_view.begin() + r.n_to_match);
    for (int k = 0; k < r.n_to_match; k++) {
        mpptr pMP = T.point(in_view[k]);
        if (!pMP) continue;
        pMP->IncreaseVisible();
        pMP->mbTrackInView = true; pMP->mTrackProjX = px[k]; pMP->mTrackProjY = py[k]; pMP->mnTrackScaleLevel = level[k]; pMP->mTrackViewCos = vc[k];
    }
    // ... and of ORBmatcher.cpp:141-143: the new matches
    for (int i = 0; i < F.N; i++) if (match[i] >= 0) F.mvpMapPoints[i] = T.point(match[i]);
}

bool Tracking::TrackLocalMap()
{
    UpdateLocalMap();

    SearchLocalPoints();

    // Optimizer::PoseOptimizationClient(*mCurrentFrame) on the handle, which holds the frame's map points after the search
    Frame& F = *mCurrentFrame;
    ccm_shim::MapTable& T = ccm_shim::MapTable::get();
    ccm_map_table* table = T.flush();
    ccm_frame* h = ccm_shim::frame_handle(F);
    if (!table || !h) throw estd::infrastructure_ex();
    double pose7[7];
    float T16[16];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T16[4 * r + c] = F.mTcw.at<float>(r, c);
    ccm_pose_from_mat4f(T16, pose7);
    const double intr[4] = {Frame::fx, Frame::fy, Frame::cx, Frame::cy};
    std::vector<uint8_t> outlier(std::max(F.N, 1));
    int32_t n_inliers = 0;
    if (ccm_frame_pose_optimize_table(ccm_shim::ctx(), h, table, F.mvInvLevelSigma2.data(), (int)F.mvInvLevelSigma2.size(), intr, pose7,
                                      outlier.data(), &n_inliers))
        throw estd::infrastructure_ex();
    ccm_pose_to_mat4f(pose7, T16);
    cv::Mat Tcw(4, 4, CV_32F);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) Tcw.at<float>(r, c) = T16[4 * r + c];
    F.SetPose(Tcw);
    for (int i = 0; i < F.N; i++) F.mvbOutlier[i] = F.mvpMapPoints[i] && outlier[i];

    mnMatchesInliers = 0;
    for (int i = 0; i < F.N; i++) {                                            // :637-648
        if (F.mvpMapPoints[i] && !F.mvbOutlier[i]) {
            F.mvpMapPoints[i]->IncreaseFound();
            mnMatchesInliers++;
        }
    }
    if (mCurrentFrame->mId.first < mLastRelocFrameId.first + params::tracking::miMaxFrames && mnMatchesInliers < 50)
        return false;
    if (mnMatchesInliers < params::tracking::miTrackLocalMapInlierThres)
        return false;
    return true;
}

}  // namespace cslam
