// cslam_tracking.cpp -- drop-in bodies of cslam::Tracking::TrackReferenceKeyFrame (src/Tracking.cpp:514-556, at the end of this file),
// Tracking::SearchLocalPoints (:860-922) and Tracking::TrackLocalMap (:623-727) on the device-resident map-point table (ccm_hot.h "map-point table").  The reference visits
// every map point of the client's map on every tracked image (this fork sets mvpLocalMapPoints = mpMap->GetAllMapPoints(), :924-934)
// and calls Frame::isInFrustum on each; here the map lives in a ccm_map_table, ONE ccm_frame_search_local_points call does both loops
// and the matcher, and ONE ccm_frame_pose_optimize_table call the pose.  Tracking::TrackWithMotionModel (:569-621) is ONE
// ccm_frame_track_motion_model on the last and the current frame's handles.  Remove these four bodies from src/Tracking.cpp; the rest
// of the file stays as it is.
//
// The table is filled where the map changes, not here: INTEGRATION.md "Map-point table" lists the one-line hooks in Map::AddMapPoint
// / EraseMapPoint and MapPoint::SetWorldPos / UpdateNormalAndDepth / ComputeDistinctiveDescriptors / SetBadFlag that call
// ccm_shim::MapTable::put / erase below.  The hooks sit inside MapPoint because the raw mfMinDistance / mfMaxDistance are private
// (GetMinDistanceInvariance returns 0.8f * mfMinDistance, which cannot be divided back exactly).
#include <cslam/Tracking.h>
#include <cslam/Frame.h>
#include <cslam/KeyFrame.h>
#include <cslam/MapPoint.h>
#include <cslam/Map.h>
#include <cslam/Optimizer.h>
#include <cslam/Converter.h>
#include <cslam/ORBmatcher.h>
#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include "ccm_shim.h"
#include "fuse_steps.h"

namespace ccm_shim {

// The slot map of one client's map: slot <-> map point, filled where map points are created and erased.  Slots are handed out in
// creation order and reused after an erase.  The visiting order of SearchLocalPoints is the order of Map::mmpMapPoints (a std::map
// keyed by idpair, src/Map.cpp:416-424); it is sent again only when the set of points has changed.  The hooks run in any thread
// (LocalMapping, Communicator), so they only queue rows under the mutex; whichever thread next works on the table sends them with
// ccm_map_table_update through its own handle before its call.
// One table, a handle per thread: the tracking thread's first flush() makes the table (the root handle, in that thread's context).  Every
// other thread -- LocalMapping, LoopFinder, MapMatcher, MapMerger, each with a context of its own -- works through a thread_local view
// (ccm_map_table_attach), attached on first use.  Only the root's thread replaces the table by a bigger one; the generation number tells
// the other threads to attach again, and the old rows live for as long as a view of them does, so nobody is stopped for the growth (a
// call that runs on an old view meanwhile sees the map as it was before).  The visiting order belongs to a handle, so "order dirty" is
// kept per handle, and only a thread that searches local points sends it.
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
            mSlotOf[pMP->mId] = slot; mPoints[slot] = pMP; mOrderStamp++;
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
        mPoints[it->second] = nullptr; mFree.push_back(it->second); mSlotOf.erase(it); mOrderStamp++;
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
    // Before a call on the table: the queued rows and, with_order (SearchLocalPoints), the visiting order when the set of points changed
    // since this thread's handle last received it.  Returns the calling thread's handle: the root on the thread whose context made the
    // table, this thread's view elsewhere; nullptr when the table must grow and this is not the root's thread (the tracking thread's next
    // flush replaces it), or when a call fails.
    ccm_map_table* flush(bool with_order = false)
    {
        std::lock_guard<std::mutex> lock(mMutex);
        ccm_ctx* c = ctx();
        const int need = (int)mPoints.size();
        if (!mTable || ccm_map_table_capacity(mTable) < need) {                // grow: a new table, the last row of every live slot again
            if (mTable && c != mCtx) return nullptr;                           // a handle is destroyed on its own context's thread
            ccm_map_table* bigger = nullptr;
            if (ccm_map_table_create(c, std::max(2 * need, 65536), &bigger)) return nullptr;
            ccm_map_table_destroy(mTable);                                     // the old rows stay until the last view of them is gone
            mTable = bigger; mCtx = c; mGeneration++; mRootOrder = 0;
            std::vector<Row> all;
            for (int s = 0; s < need; s++) if (mPoints[s]) all.push_back(mRows[s]);     // bad points that still own a slot included
            all.insert(all.end(), mQueue.begin(), mQueue.end());                         // rows queued by other threads stay behind them
            mQueue.swap(all);
        }
        uint64_t* order_sent = nullptr;
        ccm_map_table* h = handle_locked(c, &order_sent);
        if (!h) return nullptr;
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
            if (ccm_map_table_update(c, h, &u)) return nullptr;                // seen by every handle's later calls (ccm_hot.h "Table views")
            mQueue.clear();
        }
        if (with_order && *order_sent != mOrderStamp) {
            std::vector<int32_t> order;
            order.reserve(mSlotOf.size());
            for (const auto& kv : mSlotOf) order.push_back(kv.second);         // ascending idpair, as mmpMapPoints
            if (ccm_map_table_set_order(c, h, (int)order.size(), order.empty() ? &mZero : order.data())) return nullptr;
            *order_sent = mOrderStamp;
        }
        return h;
    }
    // MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth for pts in one ccm_map_table_refresh: the observation lists are
    // built from GetObservations() in the map's own order without the bad keyframes (src/MapPoint.cpp:803, :952), the device reads
    // the descriptors, camera centres and scale factors from the keyframe handles and writes the table's columns, and the one download
    // gives what the MapPoint objects keep: MapPoint::StoreRefreshed (INTEGRATION.md "Map-point table") assigns mDescriptor,
    // mNormalVector, mfMinDistance and mfMaxDistance at the hook position without calling put(), and the row copy kept here is brought
    // up to date instead: no row travels a second time.  It runs on any thread, through that thread's handle on the table (flush());
    // it returns false and touches nothing before the tracking thread has made the table, when the view cannot be attached, or when a
    // keyframe has no handle in this thread's context.  Points the call cannot express stay with the reference's functions: a bad point
    // (both return at once) and a point whose observing keyframes are all bad (normal / 0).
    // After ccm_ba_solve_table_frames has written the positions of pts into the device rows and the caller has stored the same values
    // in the points (MapPoint::StoreWorldPos, no put): the row copies kept here take them, and so does every row already QUEUED for
    // one of these slots -- a row queued by any thread between the solve and the store snapshotted the old position, and the next
    // flush would send it over the new one.  Rows queued from here on read the new position from the point itself.
    void positions_on_device(const std::vector<mpptr>& pts)
    {
        std::lock_guard<std::mutex> lock(mMutex);
        std::map<int, const float*> moved;                                       // slot -> its row copy's pos
        for (const mpptr& pMP : pts) {
            if (!pMP) continue;
            const auto it = mSlotOf.find(pMP->mId);
            if (it == mSlotOf.end()) continue;
            const cv::Mat P = pMP->GetWorldPos();
            Row& row = mRows[it->second];
            for (int k = 0; k < 3; k++) row.pos[k] = P.at<float>(k);
            moved[it->second] = row.pos;
        }
        for (Row& q : mQueue) {
            const auto it = moved.find(q.slot);
            if (it != moved.end() && (q.flags & CCM_MP_LIVE)) for (int k = 0; k < 3; k++) q.pos[k] = it->second[k];
        }
    }
    // pos_on_device (after ccm_ba_solve_table_frames and positions_on_device): the rows hold the positions already, so none travels.
    bool refresh(const std::vector<mpptr>& pts, int what, KeyframeHandleOf handle_of, bool pos_on_device = false)
    {
        ccm_ctx* c = ctx();
        if (!exists()) return false;                                             // the tracking thread's first flush makes the table
        typedef cslam::Tracking::kfptr kfptr;
        std::vector<mpptr> use;
        std::vector<int32_t> obs_first(1, 0), obs_kf, obs_feat, ref_kf, ref_feat;
        std::vector<ccm_frame*> kfs;
        std::vector<kfptr> kf_ptr;
        std::map<cslam::idpair, int> kf_index;
        auto index_of = [&](const kfptr& pKF) -> int {
            const auto it = kf_index.find(pKF->mId);
            if (it != kf_index.end()) return it->second;
            ccm_frame* h = handle_of(pKF);
            if (!h) return -1;
            kf_index[pKF->mId] = (int)kfs.size(); kfs.push_back(h); kf_ptr.push_back(pKF);
            return (int)kfs.size() - 1;
        };
        for (const mpptr& pMP : pts) {
            if (!pMP || pMP->isBad()) continue;
            const std::map<kfptr, size_t> obs = pMP->GetObservations();
            if (obs.empty()) continue;
            const size_t mark = obs_kf.size();
            for (const auto& kv : obs) {
                if (kv.first->isBad()) continue;
                const int k = index_of(kv.first);
                if (k < 0) return false;
                obs_kf.push_back(k); obs_feat.push_back((int32_t)kv.second);
            }
            if (obs_kf.size() == mark) {                                         // every observing keyframe is bad
                if (what & CCM_MPR_NORMAL_DEPTH) pMP->UpdateNormalAndDepth();
                continue;
            }
            const kfptr pRef = pMP->GetReferenceKeyFrame();
            const int kr = index_of(pRef);
            if (kr < 0) return false;
            const auto itr = obs.find(pRef);
            ref_kf.push_back(kr); ref_feat.push_back(itr == obs.end() ? 0 : (int32_t)itr->second);   // observations[pRefKF] (:813)
            obs_first.push_back((int32_t)obs_kf.size());
            use.push_back(pMP);
        }
        const int n = (int)use.size();
        if (n == 0) return true;
        for (const mpptr& pMP : use) if (slot_of(pMP) < 0) put(pMP, 0.f, 0.f);  // a point not yet in the map: its slot comes first
        ccm_map_table* table = flush();                                          // rows queued earlier must not land behind the refresh
        if (!table) return false;
        std::vector<int32_t> slot(n), best(n);
        std::vector<float> pos(3 * (size_t)n), normal(3 * (size_t)n), mn(n), mx(n);
        std::vector<uint8_t> flags(n);
        for (int i = 0; i < n; i++) {
            slot[i] = slot_of(use[i]);
            const cv::Mat P = use[i]->GetWorldPos();
            for (int k = 0; k < 3; k++) pos[3 * (size_t)i + k] = P.at<float>(k);
            flags[i] = CCM_MP_LIVE | (use[i]->Observations() > 0 ? CCM_MP_HAS_OBS : 0);
        }
        const ccm_map_refresh u{n, slot.data(), pos_on_device ? nullptr : pos.data(), flags.data(), (int32_t)kfs.size(), kfs.data(), obs_first.data(),
                                obs_kf.data(), obs_feat.data(), ref_kf.data(), ref_feat.data(), what};
        ccm_map_refresh_result r{best.data(), normal.data(), mn.data(), mx.data()};
        if (ccm_map_table_refresh(c, table, &u, &r)) return false;
        std::lock_guard<std::mutex> lock(mMutex);
        for (int i = 0; i < n; i++) {
            cv::Mat D, Nv;
            if (what & CCM_MPR_DESCRIPTOR) {
                const int e = obs_first[i] + best[i];
                D = kf_ptr[obs_kf[e]]->mDescriptors.row(obs_feat[e]).clone();
            }
            if (what & CCM_MPR_NORMAL_DEPTH) Nv = (cv::Mat_<float>(3, 1) << normal[3 * (size_t)i], normal[3 * (size_t)i + 1], normal[3 * (size_t)i + 2]);
            use[i]->StoreRefreshed(D, Nv, mn[i], mx[i]);                         // empty Mat: that member stays
            Row& row = mRows[slot[i]];
            for (int k = 0; k < 3; k++) row.pos[k] = pos[3 * (size_t)i + k];
            row.flags = flags[i];
            if (!D.empty()) for (int k = 0; k < 32; k++) row.desc[k] = D.at<uint8_t>(0, k);
            if (!Nv.empty()) { for (int k = 0; k < 3; k++) row.normal[k] = normal[3 * (size_t)i + k]; row.min_dist = mn[i]; row.max_dist = mx[i]; }
        }
        return true;
    }
    // The map-point half of a loop or merge correction in one ccm_map_table_correct_frames (fuse_steps.h, correct_on_table): moved[k]
    // takes the pose of sim3_after[k], point pts[i] moves through keyframe owner[i] and UpdateNormalAndDepth runs on it with the camera
    // centres `order` prescribes.  The observation lists are built as refresh() builds them; keyframes that are only observed follow
    // the moved ones in the handle list.  The one download gives what the MapPoint objects keep: MapPoint::StoreWorldPos and
    // MapPoint::StoreRefreshed assign it without put(), and the row copies kept here are brought up to date instead.  A point whose
    // observing keyframes are all bad moves on the device and runs the reference's UpdateNormalAndDepth afterwards (normal / 0), whose
    // hook queues its row.  The keyframes' host poses stay with the caller (KeyFrame::SetPose; the handles hold the new poses already).
    // false = nothing was done: no table in this thread, a point without a slot, a keyframe without a handle, or the call failed.
    bool correct(const std::vector<cslam::Tracking::kfptr>& moved, const double* sim3_before, const double* sim3_after, const std::vector<mpptr>& pts,
                 const std::vector<int32_t>& owner, int order, KeyframeHandleOf handle_of)
    {
        ccm_ctx* c = ctx();
        if (!exists() || pts.size() != owner.size()) return false;
        typedef cslam::Tracking::kfptr kfptr;
        std::vector<int32_t> obs_first(1, 0), obs_kf, obs_feat, ref_kf, ref_feat;
        std::vector<ccm_frame*> kfs;
        std::map<cslam::idpair, int> kf_index;
        auto index_of = [&](const kfptr& pKF) -> int {
            const auto it = kf_index.find(pKF->mId);
            if (it != kf_index.end()) return it->second;
            ccm_frame* h = handle_of(pKF);
            if (!h) return -1;
            kf_index[pKF->mId] = (int)kfs.size(); kfs.push_back(h);
            return (int)kfs.size() - 1;
        };
        for (const kfptr& pKF : moved) if (index_of(pKF) < 0) return false;
        if (kfs.size() != moved.size()) return false;                            // a keyframe twice
        const int n = (int)pts.size(), n_moved = (int)moved.size();
        std::vector<uint8_t> all_bad(n, 0);
        for (int i = 0; i < n; i++) {
            const mpptr& pMP = pts[i];
            if (!pMP || pMP->isBad() || owner[i] < 0 || owner[i] >= n_moved || slot_of(pMP) < 0) return false;
            const std::map<kfptr, size_t> obs = pMP->GetObservations();
            const size_t mark = obs_kf.size();
            for (const auto& kv : obs) {
                if (kv.first->isBad()) continue;
                const int k = index_of(kv.first);
                if (k < 0) return false;
                obs_kf.push_back(k); obs_feat.push_back((int32_t)kv.second);
            }
            int kr = 0, fr = 0;
            if (obs_kf.size() > mark) {
                const kfptr pRef = pMP->GetReferenceKeyFrame();
                if ((kr = index_of(pRef)) < 0) return false;
                const auto itr = obs.find(pRef);
                fr = itr == obs.end() ? 0 : (int32_t)itr->second;                // observations[pRefKF] (src/MapPoint.cpp:813)
            } else all_bad[i] = obs.empty() ? 0 : 1;
            ref_kf.push_back(kr); ref_feat.push_back(fr);
            obs_first.push_back((int32_t)obs_kf.size());
        }
        ccm_map_table* table = flush();                                          // rows queued earlier must not land behind the correction
        if (!table) return false;
        std::vector<int32_t> slot(std::max(n, 1));
        for (int i = 0; i < n; i++) slot[i] = slot_of(pts[i]);
        std::vector<float> pos(3 * (size_t)n + 3), normal(3 * (size_t)n + 3), mn(n + 1), mx(n + 1);
        const ccm_map_correct u{(int32_t)kfs.size(), kfs.data(), n_moved, CCM_MC_SIM3, order, sim3_before, sim3_after, nullptr, nullptr, n, slot.data(),
                                owner.data(), obs_first.data(), obs_kf.data(), obs_feat.data(), ref_kf.data(), ref_feat.data(), pos.data(),
                                normal.data(), mn.data(), mx.data()};
        if (ccm_map_table_correct_frames(c, table, &u)) return false;
        {
            std::lock_guard<std::mutex> lock(mMutex);
            for (int i = 0; i < n; i++) {
                cv::Mat Xw = (cv::Mat_<float>(3, 1) << pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]);
                pts[i]->StoreWorldPos(Xw);
                Row& row = mRows[slot[i]];
                for (int k = 0; k < 3; k++) row.pos[k] = pos[3 * (size_t)i + k];
                for (Row& q : mQueue) if (q.slot == slot[i] && (q.flags & CCM_MP_LIVE)) for (int k = 0; k < 3; k++) q.pos[k] = row.pos[k];
                if (obs_first[i + 1] == obs_first[i]) continue;
                cv::Mat Nv = (cv::Mat_<float>(3, 1) << normal[3 * (size_t)i], normal[3 * (size_t)i + 1], normal[3 * (size_t)i + 2]);
                pts[i]->StoreRefreshed(cv::Mat(), Nv, mn[i], mx[i]);             // empty Mat: the descriptor stays
                for (int k = 0; k < 3; k++) row.normal[k] = normal[3 * (size_t)i + k];
                row.min_dist = mn[i]; row.max_dist = mx[i];
            }
        }
        for (int i = 0; i < n; i++) if (all_bad[i]) pts[i]->UpdateNormalAndDepth();
        return true;
    }
    // ORBmatcher::Fuse up to the selection for every (keyframe, point) pair in one ccm_fuse_select_table_frames (fuse_steps.h,
    // fuse_select_on_table).  As refresh(): on any thread through its own handle, rows queued earlier are flushed first, and on any
    // failure nothing of the caller's is touched.
    bool fuse_select(const std::vector<cslam::Tracking::kfptr>& kfs, const std::vector<FusePose>& poses, const std::vector<mpptr>& pts, float th,
                     int chi2_check, int accept_th, KeyframeHandleOf handle_of, std::vector<int32_t>& best)
    {
        ccm_ctx* c = ctx();
        if (!exists()) return false;
        const int n_kf = (int)kfs.size(), n = (int)pts.size();
        if (poses.size() != kfs.size()) return false;
        std::vector<int32_t> slot, row_of(n, -1);
        std::vector<uint8_t> skip;
        std::map<int, int> at;                                                   // slot -> its place in the list
        for (int i = 0; i < n; i++) {
            const mpptr& pMP = pts[i];
            if (!pMP) continue;                                                  // :874
            const int s = slot_of(pMP);
            if (s < 0) return false;
            const auto it = at.find(s);
            if (it != at.end()) { row_of[i] = it->second; continue; }
            at[s] = row_of[i] = (int)slot.size();
            slot.push_back(s);
            skip.push_back(chi2_check && pMP->mbDoNotReplace ? 1 : 0);           // :880; commented out at :1026
        }
        const int m = (int)slot.size();
        std::vector<int32_t> sel((size_t)n_kf * m, -1);
        if (n_kf > 0 && m > 0) {
            std::vector<ccm_fuse_view> views(n_kf);
            for (int k = 0; k < n_kf; k++) {
                const cslam::Tracking::kfptr& pKF = kfs[k];
                ccm_fuse_view& V = views[k];
                if (!(V.kf = handle_of(pKF))) return false;
                for (int r = 0; r < 3; r++) {
                    for (int cc = 0; cc < 3; cc++) V.Tcw[4 * r + cc] = poses[k].Rcw.at<float>(r, cc);
                    V.Tcw[4 * r + 3] = poses[k].tcw.at<float>(r);
                    V.Ow[r] = poses[k].Ow.at<float>(r);
                }
                V.fx = pKF->fx; V.fy = pKF->fy; V.cx = pKF->cx; V.cy = pKF->cy;
                V.min_x = pKF->mnMinX; V.max_x = pKF->mnMaxX; V.min_y = pKF->mnMinY; V.max_y = pKF->mnMaxY;
            }
            ccm_map_table* table = flush();                                      // SetBadFlag / SetWorldPos rows queued by other threads
            if (!table) return false;
            const cslam::Tracking::kfptr& pKF0 = kfs[0];                         // one client's keyframes share the extractor's scale tables
            const ccm_fuse_table_problem p{n_kf, views.data(), m, slot.data(), skip.data(), pKF0->mfLogScaleFactor, (int32_t)pKF0->mvScaleFactors.size(),
                                           pKF0->mvScaleFactors.data(), pKF0->mvInvLevelSigma2.data(), th, chi2_check, accept_th};
            ccm_fuse_table_result r{sel.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0};
            if (ccm_fuse_select_table_frames(c, table, &p, &r)) return false;
        }
        best.assign((size_t)n_kf * n, -1);
        for (int k = 0; k < n_kf; k++)
            for (int i = 0; i < n; i++)
                if (row_of[i] >= 0) best[(size_t)k * n + i] = sel[(size_t)k * m + row_of[i]];
        return true;
    }
    // The calling thread's handle on the table, flushed: the root on the thread whose context made it, a thread_local view elsewhere.
    // nullptr before the tracking thread has made the table or when the view cannot be attached: ComputeSim3's matchers on handles
    // (cslam_sim3solver.cpp) then take the array route.
    ccm_map_table* here() { return exists() ? flush() : nullptr; }
    // The slots in view of the previous SearchLocalPoints: Frame::isInFrustum clears mbTrackInView of every point it tests, so a
    // point that was in view and is rejected now must not keep a stale `true`.
    std::vector<int32_t> mLastInView;

private:
    // A thread's view of the table, destroyed with the thread (on an orphan too, should the thread's context have gone first)
    struct View {
        ccm_map_table* t = nullptr; uint64_t generation = 0, order = 0;
        ~View() { ccm_map_table_destroy(t); }
    };
    bool exists()
    {
        std::lock_guard<std::mutex> lock(mMutex);
        return mTable != nullptr;
    }
    // mMutex held.  The handle of the thread whose context is c, and where that handle's order stamp is kept.
    ccm_map_table* handle_locked(ccm_ctx* c, uint64_t** order_sent)
    {
        if (c == mCtx) { *order_sent = &mRootOrder; return mTable; }
        static thread_local View v;
        if (v.t && v.generation != mGeneration) { ccm_map_table_destroy(v.t); v.t = nullptr; }       // the table was replaced by a bigger one
        if (!v.t) {
            if (ccm_map_table_attach(c, mTable, &v.t)) return nullptr;
            v.generation = mGeneration; v.order = 0;
        }
        *order_sent = &v.order;
        return v.t;
    }
    struct Row { int slot; float pos[3], normal[3], min_dist, max_dist; uint8_t desc[32]; uint8_t flags; };
    std::mutex mMutex;
    std::map<cslam::idpair, int> mSlotOf;
    std::vector<mpptr> mPoints;
    std::vector<int> mFree;
    std::vector<Row> mQueue, mRows;                       // mRows: the last row sent for a slot, with the raw distances
    ccm_map_table* mTable = nullptr;
    ccm_ctx* mCtx = nullptr;                              // the context of the thread that made mTable (the root handle)
    uint64_t mGeneration = 0;                             // changes whenever flush() replaces the table by a bigger one
    uint64_t mOrderStamp = 1, mRootOrder = 0;             // the set of points changed <=> a handle's order stamp differs from mOrderStamp
    int32_t mZero = 0;
};

bool refresh_map_points(const std::vector<ORBmatcher::mpptr>& pts, int what, KeyframeHandleOf handle_of, bool pos_on_device)
{
    return MapTable::get().refresh(pts, what, handle_of, pos_on_device);
}

void map_positions_on_device(const std::vector<ORBmatcher::mpptr>& pts) { MapTable::get().positions_on_device(pts); }

bool correct_on_table(const std::vector<ORBmatcher::kfptr>& moved, const double* sim3_before, const double* sim3_after,
                      const std::vector<ORBmatcher::mpptr>& pts, const std::vector<int32_t>& owner, int order, KeyframeHandleOf handle_of)
{
    return MapTable::get().correct(moved, sim3_before, sim3_after, pts, owner, order, handle_of);
}

bool correct_keyframes_on_table(const std::vector<KeyframeCorrection>& corrected, const std::function<bool(const ORBmatcher::mpptr&)>& tagged,
                                const std::function<void(const ORBmatcher::mpptr&)>& tag, KeyframeHandleOf handle_of)
{
    const int n_kf = (int)corrected.size();
    std::vector<ORBmatcher::kfptr> moved(n_kf);
    std::vector<double> before(8 * (size_t)n_kf + 8), after(8 * (size_t)n_kf + 8);
    std::vector<ORBmatcher::mpptr> pts;
    std::vector<int32_t> owner;
    std::set<cslam::idpair> taken;                                               // what the reference's tag does within one pass
    for (int k = 0; k < n_kf; k++) {
        moved[k] = corrected[k].pKF;
        std::memcpy(&before[8 * (size_t)k], corrected[k].before, 64); std::memcpy(&after[8 * (size_t)k], corrected[k].after, 64);
        const std::vector<ORBmatcher::mpptr> vpMPsi = corrected[k].pKF->GetMapPointMatches();
        for (const ORBmatcher::mpptr& pMPi : vpMPsi) {                           // src/LoopFinder.cpp:577-585
            if (!pMPi || pMPi->isBad() || tagged(pMPi) || !taken.insert(pMPi->mId).second) continue;
            pts.push_back(pMPi); owner.push_back(k);
        }
    }
    if (!MapTable::get().correct(moved, before.data(), after.data(), pts, owner, CCM_MC_IN_ORDER, handle_of)) return false;
    for (const ORBmatcher::mpptr& pMP : pts) tag(pMP);                           // :594-595
    for (int k = 0; k < n_kf; k++) {                                             // :599-608; the handle holds this pose already
        const double* S = corrected[k].after;
        const double is = 1.0 / S[7];
        const double pose7[7] = { S[0], S[1], S[2], S[3], S[4] * is, S[5] * is, S[6] * is };
        float Tcw[12], Ow[3];
        ccm_pose_to_camera(pose7, Tcw, Ow);
        cv::Mat T = cv::Mat::eye(4, 4, CV_32F);
        for (int r = 0; r < 3; r++) for (int cc = 0; cc < 4; cc++) T.at<float>(r, cc) = Tcw[4 * r + cc];
        corrected[k].pKF->SetPose(T, true);
    }
    return true;
}

int map_slot_of(const ORBmatcher::mpptr& pMP) { return pMP ? MapTable::get().slot_of(pMP) : -1; }

ccm_map_table* map_table_here() { return MapTable::get().here(); }

bool fuse_select_on_table(const std::vector<ORBmatcher::kfptr>& kfs, const std::vector<FusePose>& poses, const std::vector<ORBmatcher::mpptr>& pts,
                          float th, int chi2_check, int accept_th, KeyframeHandleOf handle_of, std::vector<int32_t>& best)
{
    return MapTable::get().fuse_select(kfs, poses, pts, th, chi2_check, accept_th, handle_of, best);
}

// One relocalisation candidate from the PnP pose to the verdict (ccm_frame_relocalize_candidate; fuse_steps.h, INTEGRATION.md
// "Relocalisation").  vpMapPointMatches / vbInliers are the candidate's SearchByBoW matches and what PnPsolver::iterate marked.  On
// return F.mvpMapPoints and F.mvbOutlier are what the stages left, nGood their last count, and with `true` F's pose is the optimised one.
bool relocalize(cslam::Frame& F, const ORBmatcher::kfptr& pKF, const cv::Mat& Tcw, const std::vector<ORBmatcher::mpptr>& vpMapPointMatches,
                const std::vector<bool>& vbInliers, KeyframeHandleOf handle_of, bool& bMatch, int& nGood)
{
    MapTable& T = MapTable::get();
    ccm_frame* cur = frame_handle(F);
    ccm_frame* kf = handle_of ? handle_of(pKF) : nullptr;
    ccm_map_table* table = cur && kf ? T.flush() : nullptr;
    if (!cur || !kf || !table || Tcw.empty() || vbInliers.size() != vpMapPointMatches.size() || (int)vbInliers.size() != F.N) return false;
    std::vector<int32_t> feature, slot;
    for (int i = 0; i < F.N; i++) {
        if (!vbInliers[i] || !vpMapPointMatches[i]) continue;
        const int s = T.slot_of(vpMapPointMatches[i]);
        if (s < 0) return false;                                               // a point without a slot: the caller takes the array route
        feature.push_back(i); slot.push_back(s);
    }
    float T16[16];
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) T16[4 * r + c] = Tcw.at<float>(r, c);
    const double intr[4] = { cslam::Frame::fx, cslam::Frame::fy, cslam::Frame::cx, cslam::Frame::cy };
    ccm_reloc_params p{};
    p.Tcw = T16; p.n_matched = (int32_t)feature.size(); p.feature = feature.data(); p.slot = slot.data();
    p.intr = intr; p.inv_level_sigma2 = F.mvInvLevelSigma2.data();
    p.view.fx = cslam::Frame::fx; p.view.fy = cslam::Frame::fy; p.view.cx = cslam::Frame::cx; p.view.cy = cslam::Frame::cy;
    p.view.min_x = cslam::Frame::mnMinX; p.view.max_x = cslam::Frame::mnMaxX; p.view.min_y = cslam::Frame::mnMinY; p.view.max_y = cslam::Frame::mnMaxY;
    p.view.n_levels = F.mnScaleLevels; p.view.scale_factors = F.mvScaleFactors.data(); p.view.log_scale_factor = F.mfLogScaleFactor;
    p.min_good = 10; p.enough = 50; p.narrow_above = 30; p.th1 = 10.f; p.dist1 = 100; p.th2 = 3.f; p.dist2 = 64; p.check_ori = 1;
    std::vector<int32_t> ids(std::max(F.N, 1), -1);
    std::vector<uint8_t> outlier(std::max(F.N, 1), 0);
    ccm_reloc_result r{};
    r.mp_id = ids.data(); r.outlier = outlier.data();
    if (ccm_frame_relocalize_candidate(ctx(), cur, kf, table, &p, &r)) return false;      // the handle's ids are as on entry
    for (int i = 0; i < F.N; i++) {
        F.mvpMapPoints[i] = ids[i] >= 0 ? T.point(ids[i]) : nullptr;
        F.mvbOutlier[i] = outlier[i] != 0;
    }
    float T16o[16];
    ccm_pose_to_mat4f(r.pose7, T16o);
    cv::Mat Tout(4, 4, CV_32F);
    std::memcpy(Tout.ptr<float>(), T16o, sizeof T16o);
    F.SetPose(Tout);
    bMatch = r.success != 0; nGood = r.n_good;
    return true;
}

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
    ccm_map_table* table = T.flush(/*with_order=*/true);
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

// ---- Tracking::TrackWithMotionModel (:569-621): UpdateLastFrame and the pose product stay on the host in cv::Mat; the clear, both
// SearchByProjection(Current, Last) passes, PoseOptimizationClient and "discard outliers" are ONE ccm_frame_track_motion_model on the
// two frames' handles and the table.  Nothing of the map is uploaded: the last frame's points travel as slots (4 bytes a feature,
// into its handle), the projection is made on the device from the table's rows.
namespace {

// CCM_SHIM_TRACK_MOTION_MODEL=0: back to the three calls (A/B timing of the two routes)
bool track_motion_model_on()
{
    static const bool on = !(getenv("CCM_SHIM_TRACK_MOTION_MODEL") && atoi(getenv("CCM_SHIM_TRACK_MOTION_MODEL")) == 0);
    return on;
}

}  // namespace

bool Tracking::TrackWithMotionModel()
{
    UpdateLastFrame();
    Frame& F = *mCurrentFrame;
    const Frame& L = *mLastFrame;
    F.SetPose(mVelocity * L.mTcw);
    const int N = F.N;
    std::fill(F.mvpMapPoints.begin(), F.mvpMapPoints.end(), mpptr());

    // The route before ccm_frame_track_motion_model: the matcher drop-in (cslam_orbmatcher.cpp: the projection on the host, valid / u / v
    // / descriptors / flags uploaded per pass), the pose drop-in, and the discard here.
    auto three_calls = [&]() -> bool {
        ORBmatcher matcher(0.9, true);
        const int th = 7;
        int nmatches = matcher.SearchByProjection(F, L, th);
        if (nmatches < 20) {
            std::fill(F.mvpMapPoints.begin(), F.mvpMapPoints.end(), mpptr());
            nmatches = matcher.SearchByProjection(F, L, 2 * th);
        }
        if (nmatches < params::tracking::miTrackWithMotionModelInlierThresSearch) return false;
        Optimizer::PoseOptimizationClient(F);
        int nmatchesMap = 0;
        for (int i = 0; i < N; i++) {
            mpptr pMP = F.mvpMapPoints[i];
            if (!pMP) continue;
            if (F.mvbOutlier[i]) {
                F.mvpMapPoints[i] = nullptr; F.mvbOutlier[i] = false;
                pMP->mbTrackInView = false; pMP->mLastFrameSeen = F.mId;
            } else if (pMP->Observations() > 0)
                nmatchesMap++;
        }
        return nmatchesMap >= params::tracking::miTrackWithMotionModelInlierThresOpt;
    };
    if (!track_motion_model_on()) return three_calls();

    ccm_ctx* c = ccm_shim::ctx();
    ccm_shim::MapTable& T = ccm_shim::MapTable::get();
    ccm_map_table* table = T.flush();
    if (!table) throw estd::infrastructure_ex();
    // (flush() gave this thread's own handle on the table -- a view where another thread's flush made it --, so the frame handles of
    // this thread's context can be used with it.)
    // Fallback: a point of the last frame has no slot (one that Map::AddMapPoint's hook never saw): the handle could not name it.
    std::vector<int32_t> slots(std::max(L.N, 1), -1);
    std::vector<uint8_t> last_outlier(std::max(L.N, 1), 0);
    for (int i = 0; i < L.N; i++) {
        last_outlier[i] = L.mvbOutlier[i] ? 1 : 0;
        if (!L.mvpMapPoints[i]) continue;
        slots[i] = T.slot_of(L.mvpMapPoints[i]);
        if (slots[i] < 0) return three_calls();
    }
    ccm_frame* hc = ccm_shim::frame_handle(F);
    ccm_frame* hl = ccm_shim::frame_handle(L);
    if (!hc || !hl || ccm_frame_set_map_points(hl, slots.data())) throw estd::infrastructure_ex();

    ccm_tmm_params p{};
    float T16[16];
    for (int r = 0; r < 4; r++) for (int cc = 0; cc < 4; cc++) T16[4 * r + cc] = F.mTcw.at<float>(r, cc);
    for (int k = 0; k < 12; k++) p.Tcw[k] = T16[k];
    p.fx = Frame::fx; p.fy = Frame::fy; p.cx = Frame::cx; p.cy = Frame::cy;
    p.min_x = Frame::mnMinX; p.max_x = Frame::mnMaxX; p.min_y = Frame::mnMinY; p.max_y = Frame::mnMaxY;
    p.n_levels = F.mnScaleLevels; p.scale_factors = F.mvScaleFactors.data();
    p.th = 7.f; p.retry_below = 20; p.min_matches = params::tracking::miTrackWithMotionModelInlierThresSearch;
    p.check_ori = 1; p.orb_dist = ORBmatcher::TH_HIGH;                         // ORBmatcher matcher(0.9, true)
    p.last_outlier = last_outlier.data();
    const double intr[4] = {Frame::fx, Frame::fy, Frame::cx, Frame::cy};
    p.inv_level_sigma2 = F.mvInvLevelSigma2.data(); p.intr = intr;
    std::vector<int32_t> match(std::max(N, 1), -1), ids(std::max(N, 1), -1);
    std::vector<uint8_t> outlier(std::max(N, 1), 0);
    ccm_tmm_result r{};
    ccm_pose_from_mat4f(T16, r.pose7);
    r.match = match.data(); r.mp_id = ids.data(); r.outlier = outlier.data();
    if (ccm_frame_track_motion_model(c, hc, hl, table, &p, &r)) throw estd::infrastructure_ex();

    for (int i = 0; i < N; i++) F.mvpMapPoints[i] = ids[i] >= 0 ? T.point(ids[i]) : mpptr();
    if (!r.posed) return false;                                                // :593: the matches stay in mvpMapPoints
    ccm_pose_to_mat4f(r.pose7, T16);
    cv::Mat Tcw(4, 4, CV_32F);
    for (int rr = 0; rr < 4; rr++) for (int cc = 0; cc < 4; cc++) Tcw.at<float>(rr, cc) = T16[4 * rr + cc];
    F.SetPose(Tcw);
    for (int i = 0; i < N; i++) {                                              // :605-612 for the points the device discarded
        if (match[i] < 0) continue;
        F.mvbOutlier[i] = false;
        if (!outlier[i]) continue;
        if (mpptr pMP = T.point(slots[match[i]])) { pMP->mbTrackInView = false; pMP->mLastFrameSeen = F.mId; }
    }
    return r.n_matches_map >= params::tracking::miTrackWithMotionModelInlierThresOpt;
}

// ---- Tracking::TrackReferenceKeyFrame (:514-556) on handles: Frame::ComputeBoW, SearchByBoW(mpReferenceKF, Frame) and
// PoseOptimizationClient run on the current frame's handle and a handle of the reference keyframe kept in this thread's context.
// Map points travel as slots of the map-point table, as in TrackLocalMap.
namespace {

// The reference keyframe's handle in the tracking thread's context.  mpReferenceKF changes at keyframe rate, so one cached handle
// serves many frames; its features and FeatureVector never change, its map-point matches are sent again on every use.
struct ReferenceHandle {
    idpair id{~(size_t)0, ~(size_t)0};
    ccm_frame* f = nullptr;
    ~ReferenceHandle() { ccm_frame_destroy(f); }
};

ccm_frame* reference_handle(const Tracking::kfptr& pKF)
{
    static thread_local ReferenceHandle R;
    if (R.f && R.id == pKF->mId) return R.f;
    ccm_frame_destroy(R.f);
    R.f = nullptr;
    const int n = (int)pKF->mvKeysUn.size();
    std::vector<float> kx(n), ky(n), angle(n); std::vector<int32_t> oct(n);
    for (int i = 0; i < n; i++) { kx[i] = pKF->mvKeysUn[i].pt.x; ky[i] = pKF->mvKeysUn[i].pt.y; oct[i] = pKF->mvKeysUn[i].octave; angle[i] = pKF->mvKeysUn[i].angle; }
    const cv::Mat desc = pKF->mDescriptors.isContinuous() ? pKF->mDescriptors : pKF->mDescriptors.clone();
    const ccm_frame_grid g{n, kx.data(), ky.data(), oct.data(), desc.data, (float)pKF->mnMinX, (float)pKF->mnMinY, pKF->mfGridElementWidthInv,
                           pKF->mfGridElementHeightInv, pKF->mnGridCols, pKF->mnGridRows};
    const std::vector<int32_t> node = ccm_shim::nodes_of(pKF->mFeatVec, n);      // KeyFrame::ComputeBoW has run in its constructor's caller
    if (ccm_frame_create(ccm_shim::ctx(), &g, angle.data(), &R.f) || ccm_frame_set_bow(R.f, node.data())) {
        ccm_frame_destroy(R.f);
        R.f = nullptr;
        return nullptr;
    }
    R.id = pKF->mId;
    return R.f;
}

}  // namespace

bool Tracking::TrackReferenceKeyFrame()
{
    Frame& F = *mCurrentFrame;
    ccm_ctx* c = ccm_shim::ctx();
    ccm_shim::MapTable& T = ccm_shim::MapTable::get();
    ccm_map_table* table = T.flush();
    ccm_vocabulary* voc = ccm_shim::vocabulary();
    ccm_frame* h = ccm_shim::frame_handle(F);
    ccm_frame* hk = reference_handle(mpReferenceKF);
    if (!table || !voc || !h || !hk) throw estd::infrastructure_ex();

    // mCurrentFrame->ComputeBoW() (:517, src/Frame.cpp:268-275): the descent and the FeatureVector order on the handle; the
    // per-feature results fill the Frame's own mBowVec / mFeatVec, which relocalisation and keyframe creation read later
    const int N = F.N;
    std::vector<int32_t> word(std::max(N, 1)), node(std::max(N, 1));
    std::vector<double> weight(std::max(N, 1));
    if (ccm_frame_compute_bow(c, h, voc, 4, word.data(), weight.data(), node.data())) throw estd::infrastructure_ex();
    if (F.mBowVec.empty()) {
        ccm_shim::VocabularyArrays& V = ccm_shim::vocabulary_arrays();
        std::vector<int32_t> ids(std::max(N, 1)), fv(std::max(N, 1));
        std::vector<double> vals(std::max(N, 1));
        const int m = ccm_bow_vector(N, word.data(), weight.data(), node.data(), V.weighting, V.scoring, ids.data(), vals.data(), fv.data());
        if (m < 0) throw estd::infrastructure_ex();
        for (int i = 0; i < m; i++) F.mBowVec.insert(F.mBowVec.end(), std::make_pair(ids[i], vals[i]));
        for (int i = 0; i < N; i++) if (fv[i] >= 0) F.mFeatVec.addFeature(fv[i], i);
    }

    // SearchByBoW(mpReferenceKF, *mCurrentFrame, vpMapPointMatches) (:521-524): the keyframe's good map points as table slots
    const std::vector<mpptr> mps = mpReferenceKF->GetMapPointMatches();
    const int n1 = (int)mps.size();
    std::vector<int32_t> slots(std::max(n1, 1), -1);
    std::vector<uint8_t> valid1(std::max(n1, 1), 0);
    for (int i = 0; i < n1; i++) {
        if (!mps[i] || mps[i]->isBad()) continue;
        valid1[i] = 1;
        slots[i] = T.slot_of(mps[i]);                                         // every point of the client's map has one (Map::AddMapPoint's hook)
    }
    if (ccm_frame_set_map_points(hk, slots.data())) throw estd::infrastructure_ex();
    const ccm_bow_options o{0.7f, 1, 50, /*strict_th=*/0};                     // ORBmatcher matcher(0.7, true), TH_LOW
    std::vector<int32_t> match(std::max(N, 1), -1);
    int nmatches = ccm_frame_search_by_bow(c, hk, h, &o, valid1.data(), params::tracking::miTrackWithRefKfInlierThresSearch, match.data());
    if (nmatches < 0) throw estd::infrastructure_ex();
    if (nmatches < params::tracking::miTrackWithRefKfInlierThresSearch)        // :526: the handle's mp_id is untouched too
        return false;

    for (int i = 0; i < N; i++) F.mvpMapPoints[i] = match[i] >= 0 ? mps[match[i]] : mpptr();     // :529 (the handle holds the slots already)
    F.SetPose(mLastFrame->mTcw);

    // Optimizer::PoseOptimizationClient(*mCurrentFrame) (:532) on the handle and the table
    double pose7[7];
    float T16[16];
    for (int r = 0; r < 4; r++) for (int cc = 0; cc < 4; cc++) T16[4 * r + cc] = F.mTcw.at<float>(r, cc);
    ccm_pose_from_mat4f(T16, pose7);
    const double intr[4] = {Frame::fx, Frame::fy, Frame::cx, Frame::cy};
    std::vector<uint8_t> outlier(std::max(N, 1));
    int32_t n_inliers = 0;
    if (ccm_frame_pose_optimize_table(c, h, table, F.mvInvLevelSigma2.data(), (int)F.mvInvLevelSigma2.size(), intr, pose7, outlier.data(), &n_inliers))
        throw estd::infrastructure_ex();
    ccm_pose_to_mat4f(pose7, T16);
    cv::Mat Tcw(4, 4, CV_32F);
    for (int r = 0; r < 4; r++) for (int cc = 0; cc < 4; cc++) Tcw.at<float>(r, cc) = T16[4 * r + cc];
    F.SetPose(Tcw);

    // Discard outliers (:534-553)
    int nmatchesMap = 0;
    for (int i = 0; i < N; i++) {
        if (!F.mvpMapPoints[i]) continue;
        if (outlier[i]) {
            mpptr pMP = F.mvpMapPoints[i];
            F.mvpMapPoints[i] = nullptr;
            F.mvbOutlier[i] = false;
            pMP->mbTrackInView = false;
            pMP->mLastFrameSeen = F.mId;
            nmatches--;
        } else if (F.mvpMapPoints[i]->Observations() > 0)
            nmatchesMap++;
    }
    return nmatchesMap >= params::tracking::miTrackWithRefKfInlierThresOpt;
}

}  // namespace cslam
