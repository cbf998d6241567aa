// cslam_frame.cpp -- drop-in bodies of cslam::Frame::UndistortKeyPoints (src/Frame.cpp:277-307), Frame::ComputeImageBounds
// (:309-337) and the monocular constructor (:55-101).  Remove these three bodies from src/Frame.cpp; the rest of the file stays.
//
// The two member functions forward to the host-only calls ccm_undistort_points / ccm_image_bounds: the same arithmetic as the device
// route below, so a Frame built either way has the same mvKeysUn, bit for bit (cv::undistortPoints in its classic five-iteration
// form; parity with a particular OpenCV build is not pinned).
//
// The constructor takes the device route: the extraction leaves keypoints and descriptors in device memory, and
// ccm_frame_from_extract_camera builds the frame handle from them -- undistortion, grid and all -- in one launch with nothing
// uploaded.  mvKeysUn is read back from the handle (ccm_frame_get_keypoints), and the handle goes into the thread's cache
// (ccm_shim::frame_handle_put), where the Frame-side matchers of cslam_orbmatcher.cpp and cslam_tracking.cpp find it.
// CCM_SHIM_FRAME_HANDLES=0 keeps the constructor on the host functions (and the matchers on per-call uploads).
#include <cslam/Frame.h>
#include <cslam/ORBextractor.h>
#include "ccm_shim.h"

namespace cslam {

namespace {

// mK and mDistCoef (CV_32F; four coefficients, or five when the settings file has a k3, src/Tracking.cpp:53-58)
ccm_camera camera_of(const cv::Mat& K, const cv::Mat& dist)
{
    ccm_camera cam{K.at<float>(0, 0), K.at<float>(1, 1), K.at<float>(0, 2), K.at<float>(1, 2),
                   dist.at<float>(0), dist.at<float>(1), dist.at<float>(2), dist.at<float>(3), 0.0f};
    if (dist.total() > 4) cam.k3 = dist.at<float>(4);
    return cam;
}

}  // namespace

void Frame::UndistortKeyPoints()
{
    const ccm_camera cam = camera_of(mK, mDistCoef);
    std::vector<float> x(N), y(N);
    for (int i = 0; i < N; i++) { x[i] = mvKeys[i].pt.x; y[i] = mvKeys[i].pt.y; }
    if (ccm_undistort_points(&cam, N, x.data(), y.data(), x.data(), y.data())) throw estd::infrastructure_ex();
    mvKeysUn = mvKeys;                                                     // size, angle, response, octave stay
    for (int i = 0; i < N; i++) { mvKeysUn[i].pt.x = x[i]; mvKeysUn[i].pt.y = y[i]; }
}

void Frame::ComputeImageBounds(const cv::Mat& imLeft)
{
    const ccm_camera cam = camera_of(mK, mDistCoef);
    ccm_frame_bounds b;
    if (ccm_image_bounds(&cam, imLeft.cols, imLeft.rows, FRAME_GRID_COLS, FRAME_GRID_ROWS, &b)) throw estd::infrastructure_ex();
    mnMinX = b.min_x; mnMaxX = b.max_x; mnMinY = b.min_y; mnMaxY = b.max_y;
}

Frame::Frame(const cv::Mat& imGray, const double& timeStamp, extractorptr pExtractor, vocptr pVoc, cv::Mat& K, cv::Mat& distCoef, size_t ClientId)
    : mpORBvocabulary(pVoc), mpORBextractor(pExtractor), mTimeStamp(timeStamp), mK(K.clone()), mDistCoef(distCoef.clone())
{
    mId = std::make_pair(nNextId++, ClientId);
    mnScaleLevels = mpORBextractor->GetLevels();
    mfScaleFactor = mpORBextractor->GetScaleFactor();
    mfLogScaleFactor = log(mfScaleFactor);
    mvScaleFactors = mpORBextractor->GetScaleFactors();
    mvInvScaleFactors = mpORBextractor->GetInverseScaleFactors();
    mvLevelSigma2 = mpORBextractor->GetScaleSigmaSquares();
    mvInvLevelSigma2 = mpORBextractor->GetInverseScaleSigmaSquares();

    ExtractORB(imGray);                                                    // cslam_orbextractor.cpp: the results stay on the device too
    N = (int)mvKeys.size();
    if (mvKeys.empty()) return;

    const ccm_camera cam = camera_of(mK, mDistCoef);
    if (mbInitialComputations) {                                           // once per calibration (:83-98)
        ccm_frame_bounds b;
        if (ccm_image_bounds(&cam, imGray.cols, imGray.rows, FRAME_GRID_COLS, FRAME_GRID_ROWS, &b)) throw estd::infrastructure_ex();
        mnMinX = b.min_x; mnMaxX = b.max_x; mnMinY = b.min_y; mnMaxY = b.max_y;
        mfGridElementWidthInv = b.inv_w; mfGridElementHeightInv = b.inv_h;
        fx = cam.fx; fy = cam.fy; cx = cam.cx; cy = cam.cy;
        invfx = 1.0f / fx; invfy = 1.0f / fy;
        mbInitialComputations = false;
    }

    ccm_frame* handle = nullptr;
    if (ccm_shim::frame_handles_on()) {
        // device route: the handle from the extract's own keypoints; mvKeysUn comes back from it
        const ccm_frame_bounds b{mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv};
        if (ccm_frame_from_extract_camera(ccm_shim::ctx(), 0, N, &cam, &b, FRAME_GRID_COLS, FRAME_GRID_ROWS, &handle)) throw estd::infrastructure_ex();
        std::vector<float> x(N), y(N);
        if (ccm_frame_get_keypoints(handle, x.data(), y.data())) { ccm_frame_destroy(handle); throw estd::infrastructure_ex(); }
        mvKeysUn = mvKeys;
        for (int i = 0; i < N; i++) { mvKeysUn[i].pt.x = x[i]; mvKeysUn[i].pt.y = y[i]; }
    } else {
        UndistortKeyPoints();
    }

    mvpMapPoints = std::vector<mpptr>(N, nullptr);
    mvbOutlier = std::vector<bool>(N, false);
    AssignFeaturesToGrid();                                                // mGrid for the host-side callers of GetFeaturesInArea
    if (handle) ccm_shim::frame_handle_put(*this, handle);
}

}  // namespace cslam
