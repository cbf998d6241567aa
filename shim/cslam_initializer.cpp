// cslam_initializer.cpp -- drop-in body of cslam::Initializer (src/Initializer.cpp): the constructor keeps the reference frame's
// keypoints and calibration (:29-38); Initialize (:40-117) draws the minimal sets from DUtils::Random exactly as :76-92 (SeedRandOnce(0),
// then RandomInt(0, vAvailableIndices.size()-1) eight times per iteration) and hands the raw draws to one ccm_initialize call, which
// evaluates every homography and fundamental-matrix hypothesis, chooses the model and reconstructs the motion.  The private helpers
// of the class (FindHomography, ComputeH21, CheckRT, ...) are not defined here: nothing outside src/Initializer.cpp calls them.
// The reference's header (include/cslam/Initializer.h) stays untouched; mvKeys2, mvMatches12 and mvbMatched1 are filled as in :45-59
// for a caller that inspects them, mvSets is left empty (the library expands the draws itself).
#include <cslam/Initializer.h>
#include "ccm_shim.h"

namespace cslam {

Initializer::Initializer(const Frame &ReferenceFrame, float sigma, int iterations)
{
    mK = ReferenceFrame.mK.clone();
    mvKeys1 = ReferenceFrame.mvKeysUn;
    mSigma = sigma;
    mSigma2 = sigma * sigma;
    mMaxIterations = iterations;
}

bool Initializer::Initialize(const Frame &CurrentFrame, const vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21,
                             vector<cv::Point3f> &vP3D, vector<bool> &vbTriangulated)
{
    mvKeys2 = CurrentFrame.mvKeysUn;
    mvMatches12.clear();
    mvMatches12.reserve(mvKeys2.size());
    mvbMatched1.resize(mvKeys1.size());
    for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {             // :50-59
        if (vMatches12[i] >= 0) { mvMatches12.push_back(make_pair(i, vMatches12[i])); mvbMatched1[i] = true; }
        else mvbMatched1[i] = false;
    }
    const int N = mvMatches12.size();
    const int n1 = (int)mvKeys1.size(), n2 = (int)mvKeys2.size();
    std::vector<float> kp1(2 * (size_t)n1), kp2(2 * (size_t)n2);
    for (int i = 0; i < n1; i++) { kp1[2 * i] = mvKeys1[i].pt.x; kp1[2 * i + 1] = mvKeys1[i].pt.y; }
    for (int i = 0; i < n2; i++) { kp2[2 * i] = mvKeys2[i].pt.x; kp2[2 * i + 1] = mvKeys2[i].pt.y; }
    std::vector<int32_t> matches(n1, -1);
    for (int i = 0; i < n1 && i < (int)vMatches12.size(); i++) matches[i] = vMatches12[i];

    const int iterations = mMaxIterations < 1 ? 1 : mMaxIterations;
    std::vector<int32_t> draws((size_t)iterations * 8, 0);
    DUtils::Random::SeedRandOnce(0);                                          // :76
    if (N >= 8)
        for (int it = 0; it < iterations; it++)
            for (int j = 0; j < 8; j++) draws[8 * (size_t)it + j] = DUtils::Random::RandomInt(0, N - 1 - j);      // :85, the list shrinks by one per draw

    ccm_initializer_problem pb{};
    pb.n1 = n1; pb.kp1_xy = kp1.data(); pb.n2 = n2; pb.kp2_xy = kp2.data(); pb.matches12 = matches.data();
    pb.fx = mK.at<float>(0, 0); pb.fy = mK.at<float>(1, 1); pb.cx = mK.at<float>(0, 2); pb.cy = mK.at<float>(1, 2);
    pb.sigma = mSigma; pb.max_iterations = iterations;
    pb.min_parallax = 1.0f; pb.min_triangulated = 50;                         // the arguments of :112 / :114
    pb.draws = draws.data();
    std::vector<float> p3d(3 * (size_t)(n1 > 0 ? n1 : 1), 0.0f);
    std::vector<uint8_t> tri(n1 > 0 ? n1 : 1, 0);
    ccm_initializer_result res{};
    res.p3d = p3d.data(); res.triangulated = tri.data(); res.tap = nullptr;
    if (ccm_initialize(ccm_shim::ctx(), &pb, &res)) throw estd::infrastructure_ex();
    if (!res.initialized) return false;                                       // R21, t21, vP3D and vbTriangulated stay as they were
    R21 = cv::Mat(3, 3, CV_32F);
    t21 = cv::Mat(3, 1, CV_32F);
    for (int k = 0; k < 9; k++) R21.ptr<float>()[k] = res.R21[k];
    for (int k = 0; k < 3; k++) t21.ptr<float>()[k] = res.t21[k];
    vP3D.resize(n1);
    vbTriangulated = vector<bool>(n1, false);
    for (int i = 0; i < n1; i++) {
        vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
        vbTriangulated[i] = tri[i] != 0;
    }
    return true;
}

}  // namespace cslam
