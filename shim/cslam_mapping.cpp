// cslam_mapping.cpp -- drop-in body of cslam::LocalMapping::CreateNewMapPoints (src/Mapping.cpp:284-469).  The reference calls
// SearchForTriangulation once per covisible neighbour and triangulates every matched pair with cv::Mat arithmetic and a cv::SVD; here
// the arrays of the current keyframe and of all neighbours are gathered once, ComputeF12 / ComputeSceneMedianDepth and the epipole
// stay the reference's own code, and ONE ccm_create_new_map_points call returns the list of new points in the reference's creation
// order.  The map points are then created neighbour by neighbour from first[], with CheckNewKeyFrames() asked between neighbours as at
// :314 and the side effects of :451-466 in the reference's order.  The rest of src/Mapping.cpp stays as it is: remove only this
// function's body there.
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
#include "ccm_shim.h"

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

}  // namespace

void LocalMapping::CreateNewMapPoints()
{
    int nn = 20;
    const vector<kfptr> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);
    const int n_kf = (int)vpNeighKFs.size();
    if (n_kf == 0) return;

    KfArrays cur_arrays;
    ccm_map_keyframe cur{};
    gather(mpCurrentKeyFrame, cur_arrays, cur);
    std::vector<KfArrays> arrays(n_kf);
    std::vector<ccm_map_keyframe> neighbours(n_kf);
    std::vector<float> F12(9 * (size_t)n_kf), epipole(2 * (size_t)n_kf), median_depth(n_kf);
    const cv::Mat Cw = mpCurrentKeyFrame->GetCameraCenter();
    for (int k = 0; k < n_kf; k++) {
        kfptr pKF2 = vpNeighKFs[k];
        gather(pKF2, arrays[k], neighbours[k]);
        median_depth[k] = pKF2->ComputeSceneMedianDepth(2);                 // :324
        const cv::Mat F = ComputeF12(mpCurrentKeyFrame, pKF2);              // :331
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) F12[9 * (size_t)k + 3 * r + c] = F.at<float>(r, c);
        const cv::Mat C2 = pKF2->GetRotation() * Cw + pKF2->GetTranslation();                       // ORBmatcher.cpp:708-714
        const float invz = 1.0f / C2.at<float>(2);
        epipole[2 * k] = pKF2->fx * C2.at<float>(0) * invz + pKF2->cx;
        epipole[2 * k + 1] = pKF2->fy * C2.at<float>(1) * invz + pKF2->cy;
    }
    ccm_new_points_problem pb{};
    pb.current = &cur; pb.n_kf = n_kf; pb.neighbours = neighbours.data();
    pb.F12 = F12.data(); pb.epipole = epipole.data(); pb.median_depth = median_depth.data();
    const int rows = std::max(cur.n, 1);
    std::vector<int32_t> kf(rows), idx1(rows), idx2(rows), first(n_kf + 1, 0);
    std::vector<float> x3d(3 * (size_t)rows);
    ccm_new_points_result res{};
    res.kf = kf.data(); res.idx1 = idx1.data(); res.idx2 = idx2.data(); res.x3d = x3d.data(); res.first = first.data(); res.tap = nullptr;
    if (ccm_create_new_map_points(ccm_shim::ctx(), &pb, &res) < 0) throw estd::infrastructure_ex();

    for (int k = 0; k < n_kf; k++) {
        if (k > 0 && CheckNewKeyFrames())                                   // :314
            return;
        kfptr pKF2 = vpNeighKFs[k];
        for (int row = first[k]; row < first[k + 1]; row++) {
            cv::Mat x3D = (cv::Mat_<float>(3, 1) << x3d[3 * (size_t)row], x3d[3 * (size_t)row + 1], x3d[3 * (size_t)row + 2]);
            // the side effects of :451-466, in that order
            mpptr pMP{new MapPoint(x3D, mpCurrentKeyFrame, mpMap, mClientId, mpComm, mpCC->mSysState, -1)};

            pMP->AddObservation(mpCurrentKeyFrame, idx1[row]);
            pMP->AddObservation(pKF2, idx2[row]);

            mpCurrentKeyFrame->AddMapPoint(pMP, idx1[row]);
            pKF2->AddMapPoint(pMP, idx2[row]);

            pMP->ComputeDistinctiveDescriptors();

            pMP->UpdateNormalAndDepth();

            mpMap->AddMapPoint(pMP);
            mlpRecentAddedMapPoints.push_back(pMP);

        }
    }
}

}  // namespace cslam
