// cslam_mapping.cpp -- drop-in body of cslam::LocalMapping::CreateNewMapPoints (src/Mapping.cpp:284-469).  The reference calls
// SearchForTriangulation once per covisible neighbour and triangulates every matched pair with cv::Mat arithmetic and a cv::SVD; here
// the arrays of the current keyframe and of all neighbours are gathered once, ComputeF12 / ComputeSceneMedianDepth and the epipole
// stay the reference's own code, and ONE ccm_create_new_map_points call returns the list of new points in the reference's creation
// order.  The map points are then created neighbour by neighbour from first[], with CheckNewKeyFrames() asked between neighbours as at
// :314 and the side effects of :451-466 in the reference's order.  The rest of src/Mapping.cpp stays as it is: remove only this
// function's body there.
//
// Keyframe handles (the default; CCM_SHIM_KEYFRAME_HANDLES=0 keeps the array path): the covisibility neighbourhood moves slowly, so the
// same 20 to 30 keyframes come back keyframe after keyframe.  A per-thread cache maps a keyframe id to a ccm_frame in LocalMapping's own
// context, made on first use (features, descriptors, grid, BoW nodes, camera) and kept until KeyFrame::SetBadFlag; only the map-point
// ids and the pose are sent again, when the keyframe's stamp (ccm_shim.h, INTEGRATION.md "Keyframe handles") says they changed.
// CreateNewMapPoints then calls ccm_create_new_map_points_frames.  SearchInNeighbors runs right after on the same keyframes: its
// first Fuse loop (:499-504) becomes one call of ccm_shim::fuse_into_targets (below, declared in fuse_steps.h), which makes ONE
// ccm_fuse_select_table_frames on this thread's view of the map-point table (or, where that declines, projects on the host and makes ONE
// ccm_fuse_select_batch_frames); the integrator replaces that loop in src/Mapping.cpp, the rest of the function stays the reference's.
//
// One difference in timing, none in result: the match of a later neighbour is computed before an earlier neighbour's points exist.
// It cannot see them anyway (ccm_hot.h "CreateNewMapPoints": vbMatched2 is never set, no orientation filter; a feature that wins with
// an earlier neighbour is dropped from the later ones by the library).  When CheckNewKeyFrames() ends the loop early, the remaining
// rows are simply not applied.
#include <cslam/Mapping.h>
#include <cslam/ORBmatcher.h>
#include <cslam/KeyFrame.h>
#include <cslam/MapPoint.h>
#include <cslam/Map.h>
#include <algorithm>
#include <cstdint>
#include <map>
#include "ccm_shim.h"
#include "fuse_steps.h"

namespace cslam {

namespace {

// The arrays one keyframe contributes; the ccm_map_keyframe points into them.
struct KfArrays {
    std::vector<float> x, y, Tcw, Ow;
    std::vector<int32_t> octave, node;
    std::vector<uint8_t> has_mp;
    cv::Mat desc;
};

void gather(const LocalMapping::kfptr& pKF, KfArrays& a, ccm_map_keyframe& m)
{
    const int n = pKF->N;
    a.x.resize(n); a.y.resize(n); a.octave.resize(n); a.has_mp.resize(n);
    for (int i = 0; i < n; i++) {
        const cv::KeyPoint& kp = pKF->mvKeysUn[i];
        a.x[i] = kp.pt.x; a.y[i] = kp.pt.y; a.octave[i] = kp.octave;
        a.has_mp[i] = pKF->GetMapPoint(i) ? 1 : 0;                          // :743-747, :760-764, as the function is entered
    }
    a.node = ccm_shim::nodes_of(pKF->mFeatVec, n);
    a.desc = pKF->mDescriptors.isContinuous() ? pKF->mDescriptors : pKF->mDescriptors.clone();
    const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
    a.Tcw.resize(12); a.Ow.resize(3);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) a.Tcw[4 * r + c] = R.at<float>(r, c);
        a.Tcw[4 * r + 3] = t.at<float>(r);
        a.Ow[r] = O.at<float>(r);
    }
    m.n = n; m.kp_x = a.x.data(); m.kp_y = a.y.data(); m.kp_octave = a.octave.data(); m.desc = a.desc.data;
    m.node = a.node.data(); m.has_mp = a.has_mp.data();
    m.fx = pKF->fx; m.fy = pKF->fy; m.cx = pKF->cx; m.cy = pKF->cy;
    m.Tcw = a.Tcw.data(); m.Ow = a.Ow.data();
    m.scale_factors = pKF->mvScaleFactors.data(); m.level_sigma2 = pKF->mvLevelSigma2.data();
    m.n_levels = (int32_t)pKF->mvScaleFactors.size();
}


// ---- the per-thread cache of keyframe handles
struct KfHandles {
    struct Entry { ccm_frame* f = nullptr; uint64_t stamp = 0; unsigned used = 0; };
    std::map<std::pair<size_t, size_t>, Entry> of;
    unsigned clock = 0;
    KfHandles() { (void)ccm_shim::thread_state(); }    // the context is made first, so it is destroyed after the handles
    ~KfHandles() { for (auto& kv : of) ccm_frame_destroy(kv.second.f); }
    void drop(const std::pair<size_t, size_t>& id)
    {
        const auto it = of.find(id);
        if (it == of.end()) return;
        ccm_frame_destroy(it->second.f);
        of.erase(it);
    }
};
KfHandles& kf_handles()
{
    static thread_local KfHandles h;
    return h;
}

// Once per CreateNewMapPoints / fuse_into_targets, before any handle is looked up: the handles of keyframes dropped since (SetBadFlag)
// go, and the least recently used ones above kMaxKeyframeHandles.
void sweep_keyframe_handles()
{
    KfHandles& H = kf_handles();
    for (const auto& id : ccm_shim::keyframes_dropped()) H.drop(id);
    while (H.of.size() > ccm_shim::kMaxKeyframeHandles) {
        auto oldest = H.of.begin();
        for (auto it = H.of.begin(); it != H.of.end(); ++it) if ((int)(it->second.used - oldest->second.used) < 0) oldest = it;
        H.drop(oldest->first);
    }
    H.clock++;
}

// The handle of pKF with its map-point ids and pose up to date, or nullptr on failure.  ids: feature i holds a map point <=> id >= 0;
// the value is the point's slot in the map-point table, which ccm_fuse_select_table_frames reads (IsInKeyFrame), or INT32_MAX -- an id
// outside every table -- while the point has none.  The stamp is not kept then, so the ids are sent again once the slot exists.
ccm_frame* keyframe_handle(const LocalMapping::kfptr& pKF)
{
    KfHandles& H = kf_handles();
    const int n = pKF->N;
    const std::pair<size_t, size_t> id(pKF->mId.first, pKF->mId.second);
    KfHandles::Entry& e = H.of[id];
    e.used = H.clock;
    const uint64_t now = ccm_shim::keyframe_stamp(id.first, id.second);
    bool fresh = false;
    if (!e.f) {
        std::vector<float> kx(n), ky(n), angle(n); std::vector<int32_t> oct(n);
        for (int i = 0; i < n; i++) { kx[i] = pKF->mvKeysUn[i].pt.x; ky[i] = pKF->mvKeysUn[i].pt.y; oct[i] = pKF->mvKeysUn[i].octave; angle[i] = pKF->mvKeysUn[i].angle; }
        const cv::Mat desc = pKF->mDescriptors.isContinuous() ? pKF->mDescriptors : pKF->mDescriptors.clone();
        const ccm_frame_grid g{n, kx.data(), ky.data(), oct.data(), desc.data, (float)pKF->mnMinX, (float)pKF->mnMinY, pKF->mfGridElementWidthInv,
                               pKF->mfGridElementHeightInv, pKF->mnGridCols, pKF->mnGridRows};
        const std::vector<int32_t> node = ccm_shim::nodes_of(pKF->mFeatVec, n);
        if (ccm_frame_create(ccm_shim::ctx(), &g, angle.data(), &e.f) || ccm_frame_set_bow(e.f, node.data()) ||
            ccm_frame_set_camera(e.f, pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mvScaleFactors.data(), pKF->mvLevelSigma2.data(), (int)pKF->mvScaleFactors.size())) {
            H.drop(id);                                                         // no half-made handle stays in the cache
            return nullptr;
        }
        fresh = true;
    }
    if (fresh || now == 0 || now != e.stamp) {                                  // 0: no hook ever touched it, so nothing is known
        std::vector<int32_t> ids(n);
        bool all_slotted = true;
        for (int i = 0; i < n; i++) {                                           // :743-747, :760-764, as the function is entered
            const LocalMapping::mpptr pMP = pKF->GetMapPoint(i);
            const int slot = ccm_shim::map_slot_of(pMP);
            ids[i] = !pMP ? -1 : slot >= 0 ? slot : INT32_MAX;
            if (pMP && slot < 0) all_slotted = false;
        }
        const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
        float Tcw[12], Ow[3];
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Tcw[4 * r + c] = R.at<float>(r, c);
            Tcw[4 * r + 3] = t.at<float>(r);
            Ow[r] = O.at<float>(r);
        }
        if (ccm_frame_set_map_points(e.f, ids.data()) || ccm_frame_set_pose(e.f, Tcw, Ow)) return nullptr;
        e.stamp = all_slotted ? now : 0;
    }
    return e.f;
}

}  // namespace

void LocalMapping::CreateNewMapPoints()
{
    int nn = 20;
    const vector<kfptr> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
    const int n_kf = (int)vpNeighKFs.size();
    if (n_kf == 0) return;

    const bool handles = ccm_shim::keyframe_handles_on();
    KfArrays cur_arrays;
    ccm_map_keyframe cur{};
    std::vector<KfArrays> arrays(handles ? 0 : n_kf);
    std::vector<ccm_map_keyframe> neighbours(handles ? 0 : n_kf);
    ccm_frame* hcur = nullptr;
    std::vector<ccm_frame*> hnb(n_kf, nullptr);
    if (handles) {
        sweep_keyframe_handles();
        if (!(hcur = keyframe_handle(mpCurrentKeyFrame))) throw estd::infrastructure_ex();
    } else {
        gather(mpCurrentKeyFrame, cur_arrays, cur);
    }
    const int n1 = mpCurrentKeyFrame->N;
    std::vector<float> F12(9 * (size_t)n_kf), epipole(2 * (size_t)n_kf), median_depth(n_kf);
    const cv::Mat Cw = mpCurrentKeyFrame->GetCameraCenter();
    for (int k = 0; k < n_kf; k++) {
        kfptr pKF2 = vpNeighKFs[k];
        if (handles) {
            if (!(hnb[k] = keyframe_handle(pKF2))) throw estd::infrastructure_ex();
        } else {
            gather(pKF2, arrays[k], neighbours[k]);
        }
        median_depth[k] = pKF2->ComputeSceneMedianDepth(2);                 // :324
        const cv::Mat F = ComputeF12(mpCurrentKeyFrame, pKF2);              // :331
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) F12[9 * (size_t)k + 3 * r + c] = F.at<float>(r, c);
        const cv::Mat C2 = pKF2->GetRotation() * Cw + pKF2->GetTranslation();                       // ORBmatcher.cpp:708-714
        const float invz = 1.0f / C2.at<float>(2);
        epipole[2 * k] = pKF2->fx * C2.at<float>(0) * invz + pKF2->cx;
        epipole[2 * k + 1] = pKF2->fy * C2.at<float>(1) * invz + pKF2->cy;
    }
    const int rows = std::max(n1, 1);
    std::vector<int32_t> kf(rows), idx1(rows), idx2(rows), first(n_kf + 1, 0);
    std::vector<float> x3d(3 * (size_t)rows);
    ccm_new_points_result res{};
    res.kf = kf.data(); res.idx1 = idx1.data(); res.idx2 = idx2.data(); res.x3d = x3d.data(); res.first = first.data(); res.tap = nullptr;
    if (handles) {
        ccm_new_points_frames pf{};
        pf.current = hcur; pf.n_kf = n_kf; pf.neighbours = hnb.data();
        pf.F12 = F12.data(); pf.epipole = epipole.data(); pf.median_depth = median_depth.data();
        if (ccm_create_new_map_points_frames(ccm_shim::ctx(), &pf, &res) < 0) throw estd::infrastructure_ex();
    } else {
        ccm_new_points_problem pb{};
        pb.current = &cur; pb.n_kf = n_kf; pb.neighbours = neighbours.data();
        pb.F12 = F12.data(); pb.epipole = epipole.data(); pb.median_depth = median_depth.data();
        if (ccm_create_new_map_points(ccm_shim::ctx(), &pb, &res) < 0) throw estd::infrastructure_ex();
    }

    for (int k = 0; k < n_kf; k++) {
        if (k > 0 && CheckNewKeyFrames())                                   // :314
            return;
        kfptr pKF2 = vpNeighKFs[k];
        std::vector<mpptr> created;
        created.reserve(first[k + 1] - first[k]);
        for (int row = first[k]; row < first[k + 1]; row++) {
            cv::Mat x3D = (cv::Mat_<float>(3, 1) << x3d[3 * (size_t)row], x3d[3 * (size_t)row + 1], x3d[3 * (size_t)row + 2]);
            // the side effects of :451-466, in that order
            mpptr pMP{new MapPoint(x3D, mpCurrentKeyFrame, mpMap, mClientId, mpComm, mpCC->mSysState, -1)};

            pMP->AddObservation(mpCurrentKeyFrame, idx1[row]);
            pMP->AddObservation(pKF2, idx2[row]);

            mpCurrentKeyFrame->AddMapPoint(pMP, idx1[row]);
            pKF2->AddMapPoint(pMP, idx2[row]);

            created.push_back(pMP);
        }
        // ComputeDistinctiveDescriptors and UpdateNormalAndDepth (:461-463) of this neighbour's points in one ccm_map_table_refresh on
        // the handles used above and this thread's view of the table, still in front of Map::AddMapPoint as in the reference; point by
        // point where that declines (ccm_shim::MapTable::refresh)
        if (!(handles && ccm_shim::refresh_map_points(created, CCM_MPR_DESCRIPTOR | CCM_MPR_NORMAL_DEPTH, &keyframe_handle))) {
            for (const mpptr& pMP : created) {
                pMP->ComputeDistinctiveDescriptors();

                pMP->UpdateNormalAndDepth();
            }
        }
        for (const mpptr& pMP : created) {
            mpMap->AddMapPoint(pMP);
            mlpRecentAddedMapPoints.push_back(pMP);
        }
    }
}

}  // namespace cslam

// fuse_steps.h: the cache above for the local bundle adjustment on the table (cslam_optimizer.cpp), which runs on this thread
ccm_frame* ccm_shim::local_keyframe_handle(const cslam::ORBmatcher::kfptr& pKF)
{
    using namespace cslam;
    return ccm_shim::keyframe_handles_on() ? keyframe_handle(pKF) : nullptr;
}

void ccm_shim::local_keyframe_pose_published(const cslam::ORBmatcher::kfptr& pKF, uint64_t stamp_before)
{
    using namespace cslam;
    KfHandles& H = kf_handles();
    const auto it = H.of.find(std::make_pair(pKF->mId.first, pKF->mId.second));
    if (it == H.of.end() || stamp_before == 0 || it->second.stamp != stamp_before) return;      // not up to date before: sent again on its next use
    it->second.stamp = ccm_shim::keyframe_stamp(pKF->mId.first, pKF->mId.second);
}

// The first Fuse loop of LocalMapping::SearchInNeighbors (src/Mapping.cpp:499-504) on keyframe handles.  First choice: ONE
// ccm_fuse_select_table_frames projects the current keyframe's map points into every target keyframe, gates and selects on the
// device, reading the points from the map-point table (ccm_shim::fuse_select_on_table, fuse_steps.h).  Where that is not possible --
// there is no table yet, the view cannot be attached, or a point has no slot yet -- the points are projected on the host and ONE
// ccm_fuse_select_batch_frames selects for all keyframes.  Either way a second-level neighbour can be listed twice (:486-493), and so
// can its handle, and the results are applied keyframe by keyframe in the list's order with the reference's state checks repeated at
// application time (apply_fuse).  With CCM_SHIM_KEYFRAME_HANDLES=0 it is the loop of
// ORBmatcher::Fuse calls.  Called from LocalMapping's thread only.
void ccm_shim::fuse_into_targets(const std::vector<cslam::ORBmatcher::kfptr>& vpTargetKFs, const std::vector<cslam::ORBmatcher::mpptr>& vpMapPointMatches)
{
    using namespace cslam;
    const int n_t = (int)vpTargetKFs.size(), nMPs = (int)vpMapPointMatches.size();
    if (!keyframe_handles_on() || n_t == 0 || nMPs == 0) {
        ORBmatcher matcher;
        for (const ORBmatcher::kfptr& pKFi : vpTargetKFs) matcher.Fuse(pKFi, vpMapPointMatches);
        return;
    }
    sweep_keyframe_handles();
    {
        std::vector<FusePose> poses(n_t);
        for (int k = 0; k < n_t; k++) poses[k] = FusePose{vpTargetKFs[k]->GetRotation(), vpTargetKFs[k]->GetTranslation(), vpTargetKFs[k]->GetCameraCenter()};
        std::vector<int32_t> best;
        if (fuse_select_on_table(vpTargetKFs, poses, vpMapPointMatches, 3.0f, /*chi2_check=*/1, ORBmatcher::TH_LOW, &keyframe_handle, best)) {
            for (int k = 0; k < n_t; k++) apply_fuse(vpTargetKFs[k], vpMapPointMatches, best.data() + (size_t)k * nMPs);
            return;
        }
    }
    std::vector<ccm_frame*> h(n_t);
    std::vector<int32_t> mp_first(n_t + 1, 0), level;
    std::vector<uint8_t> valid, desc;
    std::vector<float> u, v;
    for (int k = 0; k < n_t; k++) {
        const ORBmatcher::kfptr& pKFi = vpTargetKFs[k];
        if (!(h[k] = keyframe_handle(pKFi))) throw estd::infrastructure_ex();
        const FuseQuery q = project_for_fuse(pKFi, pKFi->GetRotation(), pKFi->GetTranslation(), pKFi->GetCameraCenter(), vpMapPointMatches,
                                             fuse_candidates(pKFi, vpMapPointMatches), false);
        valid.insert(valid.end(), q.valid.begin(), q.valid.end()); desc.insert(desc.end(), q.desc.begin(), q.desc.end());
        u.insert(u.end(), q.u.begin(), q.u.end()); v.insert(v.end(), q.v.begin(), q.v.end());
        level.insert(level.end(), q.level.begin(), q.level.end());
        mp_first[k + 1] = mp_first[k] + nMPs;
    }
    std::vector<int32_t> best(valid.size(), -1), dist(valid.size(), 256);
    // every keyframe of one client shares the extractor's scale tables (KeyFrame copies them from its Frame)
    const ORBmatcher::kfptr& pKF0 = vpTargetKFs[0];
    if (ccm_fuse_select_batch_frames(ctx(), n_t, h.data(), pKF0->mvScaleFactors.data(), pKF0->mvInvLevelSigma2.data(), mp_first.data(), valid.data(),
                                     u.data(), v.data(), level.data(), desc.data(), 3.0f, /*chi2_check=*/1, ORBmatcher::TH_LOW, best.data(), dist.data()))
        throw estd::infrastructure_ex();
    for (int k = 0; k < n_t; k++) apply_fuse(vpTargetKFs[k], vpMapPointMatches, best.data() + mp_first[k]);
}
