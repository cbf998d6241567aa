// fuse_steps.h -- the host steps of ORBmatcher::Fuse (ORBmatcher.cpp:854-1000) around the selection on the GPU, shared by
// cslam_orbmatcher.cpp (one keyframe per call) and cslam_mapping.cpp (the first loop of SearchInNeighbors, all target keyframes in
// one ccm_fuse_select_batch_frames call, ccm_shim::fuse_into_targets).  Include after cslam/ORBmatcher.h, cslam/KeyFrame.h and cslam/MapPoint.h.
#pragma once
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>

namespace ccm_shim {

using cslam::ORBmatcher;

// :888-927 / :1029-1066: projection, image bounds, distance range, viewing angle, predicted level
struct FuseQuery { std::vector<uint8_t> valid, desc; std::vector<float> u, v; std::vector<int32_t> level; };
inline FuseQuery project_for_fuse(const ORBmatcher::kfptr& pKF, const cv::Mat& Rcw, const cv::Mat& tcw, const cv::Mat& Ow,
                           const std::vector<ORBmatcher::mpptr>& pts, const std::vector<uint8_t>& candidate, bool invz_via_double)
{
    const int n = (int)pts.size();
    FuseQuery q; q.valid.assign(n, 0); q.desc.assign((size_t)n * 32, 0); q.u.assign(n, 0.f); q.v.assign(n, 0.f); q.level.assign(n, 0);
    const float fx = pKF->fx, fy = pKF->fy, cx = pKF->cx, cy = pKF->cy;
    for (int i = 0; i < n; i++) {
        if (!candidate[i]) continue;
        const ORBmatcher::mpptr& pMP = pts[i];
        const cv::Mat p3Dw = pMP->GetWorldPos();
        const cv::Mat p3Dc = Rcw * p3Dw + tcw;
        if (p3Dc.at<float>(2) < 0.0f) continue;
        // (:899 divides in float, `1/z`; :1041 in double, `1.0/z`, and rounds the quotient to float: kept apart, the two can differ in the last bit)
        const float invz = invz_via_double ? (float)(1.0 / p3Dc.at<float>(2)) : 1 / p3Dc.at<float>(2);
        const float u = fx * (p3Dc.at<float>(0) * invz) + cx, v = fy * (p3Dc.at<float>(1) * invz) + cy;
        if (!pKF->IsInImage(u, v)) continue;
        const float maxDistance = pMP->GetMaxDistanceInvariance(), minDistance = pMP->GetMinDistanceInvariance();
        const cv::Mat PO = p3Dw - Ow;
        const float dist3D = cv::norm(PO);
        if (dist3D < minDistance || dist3D > maxDistance) continue;
        if (PO.dot(pMP->GetNormal()) < 0.5 * dist3D) continue;
        q.level[i] = pMP->PredictScale(dist3D, pKF);
        q.u[i] = u; q.v[i] = v; q.valid[i] = 1;
        const cv::Mat d = pMP->GetDescriptor();
        if (!d.empty()) std::memcpy(&q.desc[(size_t)i * 32], d.ptr<uint8_t>(), 32);
    }
    return q;
}

// :878-886: the points Fuse looks at for keyframe pKF
inline std::vector<uint8_t> fuse_candidates(const ORBmatcher::kfptr& pKF, const std::vector<ORBmatcher::mpptr>& pts)
{
    std::vector<uint8_t> candidate(pts.size());
    for (size_t i = 0; i < pts.size(); i++) {
        const ORBmatcher::mpptr& pMP = pts[i];
        candidate[i] = pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF) && !pMP->mbDoNotReplace;
    }
    return candidate;
}

// :956-990 in map-point order: best[i] = the selected feature of pKF for point i, or -1.  Returns nFused.
inline int apply_fuse(const ORBmatcher::kfptr& pKF, const std::vector<ORBmatcher::mpptr>& pts, const int32_t* best)
{
    int nFused = 0;
    for (size_t i = 0; i < pts.size(); i++) {
        if (best[i] < 0) continue;
        const ORBmatcher::mpptr& pMP = pts[i];
        if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;                     // an earlier Replace changed this point: the reference skips it at :881
        const ORBmatcher::mpptr pMPinKF = pKF->GetMapPoint(best[i]);
        if (pMPinKF) {
            if (!pMPinKF->isBad() && !pMPinKF->mbDoNotReplace) {
                if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
                else pMPinKF->Replace(pMP);
            }
        } else {
            pMP->AddObservation(pKF, best[i]);
            pKF->AddMapPoint(pMP, best[i]);
        }
        nFused++;
    }
    return nFused;
}

// The first Fuse loop of LocalMapping::SearchInNeighbors on keyframe handles (defined in cslam_mapping.cpp; LocalMapping's thread only)
void fuse_into_targets(const std::vector<ORBmatcher::kfptr>& vpTargetKFs, const std::vector<ORBmatcher::mpptr>& vpMapPointMatches);

// MapPoint::ComputeDistinctiveDescriptors (what & CCM_MPR_DESCRIPTOR) and MapPoint::UpdateNormalAndDepth (what & CCM_MPR_NORMAL_DEPTH)
// for all of pts in one ccm_map_table_refresh on the map-point table and the caller's keyframe handles (ccm_shim::MapTable::refresh,
// defined in cslam_tracking.cpp).  handle_of returns the handle of a keyframe in the calling thread's context, camera and pose set.
// It works through the calling thread's own handle on the table (a view where another thread made it, ccm_map_table_attach).
// false = nothing was done (there is no table yet, the view cannot be attached, or a handle is missing): the caller then runs the
// reference's two functions point by point, whose hooks queue the rows.
// pos_on_device: the table's rows already hold the points' positions (ccm_ba_solve_table_frames wrote them, the caller has stored them
// with MapPoint::StoreWorldPos and told the table with map_positions_on_device): the call goes with pos = NULL.
using KeyframeHandleOf = ccm_frame* (*)(const ORBmatcher::kfptr&);
bool refresh_map_points(const std::vector<ORBmatcher::mpptr>& pts, int what, KeyframeHandleOf handle_of, bool pos_on_device = false);

// LocalMapping's cache of keyframe handles (defined in cslam_mapping.cpp; LocalMapping's thread only), for the local bundle adjustment
// on the table (cslam_optimizer.cpp).  local_keyframe_handle: the handle of pKF in that thread's context with its map-point ids,
// camera and pose up to date, or nullptr (handles switched off, or a call failed).  local_keyframe_pose_published: the device has
// written pKF's optimised pose into the handle and KeyFrame::SetPose has stored the same pose; stamp_before = the keyframe's stamp
// (ccm_shim::keyframe_stamp) read just before that SetPose.  A handle that was up to date then stays so, and no pose is uploaded.
ccm_frame* local_keyframe_handle(const ORBmatcher::kfptr& pKF);
void local_keyframe_pose_published(const ORBmatcher::kfptr& pKF, uint64_t stamp_before);

// After ccm_ba_solve_table_frames: the device rows of pts hold new positions and the caller has stored the same values in the points
// with MapPoint::StoreWorldPos (no put).  Brings the table's row copies and every row ALREADY QUEUED for these slots to those positions
// (ccm_shim::MapTable::positions_on_device, cslam_tracking.cpp), so that no flush writes an old position over a new one.  To be called
// before anything that may queue rows of these points (the erase loop's EraseObservation carries the put hook).
void map_positions_on_device(const std::vector<ORBmatcher::mpptr>& pts);

// Loop and merge corrections on the table (ccm_map_table_correct_frames; defined in cslam_tracking.cpp, INTEGRATION.md "Loop and merge
// corrections on the table").  Both work through the calling thread's handle on the table and keyframe handles of that thread's
// context (handle_of), and return false with nothing touched when there is no table here, a point has no slot, a handle is missing
// or the call fails: the caller then runs the reference's loop.
// correct_on_table: moved[k] takes the pose [R | t/s] of sim3_after[k] in its HANDLE (the caller makes KeyFrame::SetPose on the host
// object), pts[i] -- not bad, with a slot -- becomes correctedSwi.map(Siw.map(P)) through keyframe owner[i] in [0, moved.size()), and
// UpdateNormalAndDepth runs on it with the camera centres `order` (CCM_MC_POSES_FIRST / CCM_MC_IN_ORDER) prescribes.  The points take
// the results with MapPoint::StoreWorldPos / StoreRefreshed (no put), and the table's row copies and queued rows follow, so that no
// flush writes an old position over a new one.
bool correct_on_table(const std::vector<ORBmatcher::kfptr>& moved, const double* sim3_before /* [n][8] */, const double* sim3_after /* [n][8] */,
                      const std::vector<ORBmatcher::mpptr>& pts, const std::vector<int32_t>& owner, int order, KeyframeHandleOf handle_of);
// The loop of LoopFinder::CorrectLoop (src/LoopFinder.cpp:568-613) and MapMerger::MergeMaps (src/MapMerger.cpp:349-392) in one call:
// walks `corrected` in the caller's order (the iteration order of CorrectedSim3), gives each map point that is not bad and not yet
// tagged -- tagged(pMP), e.g. mCorrectedByKF_LC == mpCurrentKF->mId -- to the FIRST keyframe that carries it, issues the
// CCM_MC_IN_ORDER call, and afterwards tags the points (tag(pMP)), stores positions, normals and depths in them, and makes
// pKF->SetPose([R | t/s], true) on every keyframe.  before / after = g2oSiw / g2oCorrectedSiw as qx,qy,qz,qw,tx,ty,tz,s.
// UpdateConnections and the caller's bookkeeping (sChangedKFs) stay with the caller.
struct KeyframeCorrection { ORBmatcher::kfptr pKF; double before[8], after[8]; };
bool correct_keyframes_on_table(const std::vector<KeyframeCorrection>& corrected, const std::function<bool(const ORBmatcher::mpptr&)>& tagged,
                                const std::function<void(const ORBmatcher::mpptr&)>& tag, KeyframeHandleOf handle_of);
// The keyframe handles of a thread that is not LocalMapping's (LoopFinder, MapMerger), for the entry points that have no handle_of
// argument of their own (Optimizer::OptimizeEssentialGraph*, cslam_optimizer.cpp): the thread binds its lookup once, and
// thread_keyframe_handle gives the handle or nullptr (nothing bound, or the lookup has none).
inline KeyframeHandleOf& thread_keyframe_handles()
{
    static thread_local KeyframeHandleOf f = nullptr;
    return f;
}
inline ccm_frame* thread_keyframe_handle(const ORBmatcher::kfptr& pKF) { return thread_keyframe_handles() ? thread_keyframe_handles()(pKF) : nullptr; }

// One candidate of ORB-SLAM's Tracking::Relocalization from the PnP pose to the verdict in ONE ccm_frame_relocalize_candidate (defined in
// cslam_tracking.cpp; INTEGRATION.md "Relocalisation"): the pose optimisations, both relocalisation SearchByProjection calls and the
// outlier handling on the frame's handle, pKF's keyframe handle and the table.  false = nothing was touched: F has no handle, pKF none
// in handle_of, there is no table, or a matched point has no slot; the caller then runs the steps on the array route.
bool relocalize(cslam::Frame& F, const ORBmatcher::kfptr& pKF, const cv::Mat& Tcw, const std::vector<ORBmatcher::mpptr>& vpMapPointMatches,
                const std::vector<bool>& vbInliers, KeyframeHandleOf handle_of, bool& bMatch, int& nGood);

// The slot of pMP in the calling process's map-point table, or -1 (ccm_shim::MapTable::slot_of, cslam_tracking.cpp).  A keyframe handle
// that is to serve fuse_select_on_table carries these in its map-point ids.
int map_slot_of(const ORBmatcher::mpptr& pMP);
// The calling thread's handle on the process's map-point table with every queued row sent: the table itself on the thread whose
// context made it, a thread_local view of its rows (ccm_map_table_attach) on any other.  nullptr before the tracking thread has made
// the table or when the attach fails: the caller takes the array routes.
ccm_map_table* map_table_here();

// ComputeSim3's two matchers on keyframe handles and the table (defined in cslam_sim3solver.cpp; INTEGRATION.md "ComputeSim3 on
// handles").  Both return false with nothing touched when the table is not in the calling context, a point has no slot or a handle is
// missing: the caller then makes the reference's call, which takes the array route (cslam_orbmatcher.cpp).
// SearchBySim3(pKF1, candidates[i], vvpMatches12[i], s12[i], R12[i], t12[i], th) for every candidate in ONE call; found[i] = nFound.
bool search_by_sim3_on_table(const ORBmatcher::kfptr& pKF1, const std::vector<ORBmatcher::kfptr>& candidates,
                             std::vector<std::vector<ORBmatcher::mpptr>>& vvpMatches12, const std::vector<float>& s12, const std::vector<cv::Mat>& R12,
                             const std::vector<cv::Mat>& t12, float th, KeyframeHandleOf handle_of, std::vector<int>& found);
// SearchByProjection(pKF, Scw, vpPoints, vpMatched, th), RemapMapPointMatch (:414-435) included; nmatches = its return value.
bool search_by_projection_on_table(const ORBmatcher::kfptr& pKF, const cv::Mat& Scw, const std::vector<ORBmatcher::mpptr>& vpPoints,
                                   std::vector<ORBmatcher::mpptr>& vpMatched, int th, KeyframeHandleOf handle_of, int& nmatches);
// The Sim3Solver batch of the first loop of ComputeSim3 (src/LoopFinder.cpp:251-282) with the constructor's loop on the device: one
// ccm_sim3_solver_create_frames for the candidates' vvpMatches12, correspondences named by features.  draws: the caller's RandomInt
// results, [candidates][max_iterations][3].  n[i] = the correspondences of candidate i, those that passed src/Sim3Solver.cpp:32-59.
// Declines like its neighbours; *out is then untouched.
bool sim3_solvers_on_table(const ORBmatcher::kfptr& pKF1, const std::vector<ORBmatcher::kfptr>& candidates,
                           const std::vector<std::vector<ORBmatcher::mpptr>>& vvpMatches12, bool fix_scale, double probability, int min_inliers,
                           int max_iterations, const std::vector<int32_t>& draws, KeyframeHandleOf handle_of, std::vector<int>& n, ccm_sim3_solver** out);
// SearchBySim3 and OptimizeSim3 (src/LoopFinder.cpp:313-330, src/MapMatcher.cpp:318-333) for every candidate that returned an Scm in one
// pass, in ONE ccm_compute_sim3_table_frames: vvpMatches12[i] holds the solver's inliers on entry and vpMapPointMatches after
// OptimizeSim3 on return, sim3[i] = gScm in and out (8 doubles: qx, qy, qz, qw, tx, ty, tz, s), n_inliers[i] = OptimizeSim3's verdict.
bool compute_sim3_candidates_on_table(const ORBmatcher::kfptr& pKF1, const std::vector<ORBmatcher::kfptr>& candidates,
                                      std::vector<std::vector<ORBmatcher::mpptr>>& vvpMatches12, const std::vector<float>& s12,
                                      const std::vector<cv::Mat>& R12, const std::vector<cv::Mat>& t12, float th, float th2, bool fix_scale,
                                      KeyframeHandleOf handle_of, std::vector<double>& sim3, std::vector<int>& n_inliers);

// The projection, the gates and the selection of ORBmatcher::Fuse (:870-955, :1018-1101) for every keyframe of kfs and every point of
// pts in ONE ccm_fuse_select_table_frames on the map-point table: nothing is projected on the host and nothing is uploaded per pair.
// poses[k] = the pose Fuse would use for kfs[k]: GetRotation / GetTranslation / GetCameraCenter (:856-864), or the decomposition of
// Scw (:1004-1008).  chi2_check = 1, th = 3 is Fuse(pKF, vpMapPoints); chi2_check = 0, th = 4 is Fuse(pKF, Scw, ...), which does not
// ask mbDoNotReplace (:1026), so that flag is honoured with chi2_check only.  Every distinct point travels once; a null pointer gets
// -1 and a duplicate the row of its first occurrence (the caller's apply step re-tests IsInKeyFrame, as the reference's second visit
// would).  best [kfs.size()][pts.size()] = the selected feature or -1.
// false = nothing was done and best is untouched: the calling thread has no handle on the table (map_table_here), a point has no
// slot yet, or a handle is missing.  The caller then takes the host route (project_for_fuse and ccm_fuse_select_batch_frames).
struct FusePose { cv::Mat Rcw, tcw, Ow; };
bool fuse_select_on_table(const std::vector<ORBmatcher::kfptr>& kfs, const std::vector<FusePose>& poses, const std::vector<ORBmatcher::mpptr>& pts,
                          float th, int chi2_check, int accept_th, KeyframeHandleOf handle_of, std::vector<int32_t>& best);

}  // namespace ccm_shim
