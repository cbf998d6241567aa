// undistort.h -- Frame::UndistortKeyPoints (src/Frame.cpp:277-307) as one definition for the host entry points (ccm_undistort_points,
// ccm_image_bounds in frame_host.cpp) and for k_frame_build_batch (frame_kernels.hip): the fixed-count form of cvUndistortPoints as
// Frame.cpp:295 calls it (R empty, P = mK, the CV_32F matrices widened to double).  Every operation is one IEEE double operation in the
// order written; the library is built with -ffp-contract=off, so the host and the device compiler give the same bits.  The terms the
// reference never sets (k4..k6, thin prism, tilt) are left out; there is no guard on the sign of the denominator.
// Light header: the public header only.  It compiles as plain C++ too (a host-only test program), where the qualifiers vanish.
#pragma once
#include "../../include/ccm_hot.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CCM_UNDIST_HD __host__ __device__
#else
#define CCM_UNDIST_HD
#endif

#define CCM_UNDISTORT_ITERS 5                        // the count is part of the definition: 5 iterations are not converged

// The float values of mK / mDistCoef widened to double, and the two reciprocals every point shares
struct UndistortCam { double fx, fy, cx, cy, ifx, ify, k1, k2, p1, p2, k3; };

CCM_UNDIST_HD inline UndistortCam undistort_cam(const ccm_camera& c)
{
    UndistortCam U;
    U.fx = (double)c.fx; U.fy = (double)c.fy; U.cx = (double)c.cx; U.cy = (double)c.cy;
    U.ifx = 1.0 / U.fx; U.ify = 1.0 / U.fy;
    U.k1 = (double)c.k1; U.k2 = (double)c.k2; U.p1 = (double)c.p1; U.p2 = (double)c.p2; U.k3 = (double)c.k3;
    return U;
}

// One keypoint (u, v) -> (*uo, *vo).  One reciprocal per iteration.
CCM_UNDIST_HD inline void undistort_point(const UndistortCam& U, float u, float v, float* uo, float* vo)
{
    const double x0 = ((double)u - U.cx) * U.ifx, y0 = ((double)v - U.cy) * U.ify;
    const double tp1 = 2.0 * U.p1, tp2 = 2.0 * U.p2;
    double x = x0, y = y0;
    for (int it = 0; it < CCM_UNDISTORT_ITERS; it++) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((U.k3 * r2 + U.k2) * r2 + U.k1) * r2);
        const double dx = (tp1 * x) * y + U.p2 * (r2 + (2.0 * x) * x);
        const double dy = U.p1 * (r2 + (2.0 * y) * y) + (tp2 * x) * y;
        x = (x0 - dx) * icdist; y = (y0 - dy) * icdist;
    }
    *uo = (float)(U.fx * x + U.cx); *vo = (float)(U.fy * y + U.cy);
}
