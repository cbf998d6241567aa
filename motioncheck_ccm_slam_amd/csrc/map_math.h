// map_math.h -- the per-pair arithmetic of LocalMapping::CreateNewMapPoints (src/Mapping.cpp:312-448) and of the candidate test of
// ORBmatcher::SearchForTriangulation (ORBmatcher.cpp:768-784, CheckDistEpipolarLine :159-176).  Plain functions shared by the kernels
// (map_kernels.hip), the host (map_host.cpp) and the host check (tests/support/map_math_check.cpp).  Float storage and float
// arithmetic in the reference's operation order; the sums of cv::Mat products, dot and norm in double, stored as float; the null
// vector of the float 4x4 from the Jacobi of init_math.h in double on A^T A.  Built with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>
#include "init_math.h"

#define MAP_FN INI_FN

// CCM_NP_* of include/ccm_hot.h (this header is also compiled without it)
enum { MAP_SKIPPED_KF = 0, MAP_HAS_MP, MAP_NO_MATCH, MAP_LOW_PARALLAX, MAP_W_ZERO, MAP_NONFINITE, MAP_BEHIND_1, MAP_BEHIND_2, MAP_REPROJ_1,
       MAP_REPROJ_2, MAP_ZERO_DIST, MAP_SCALE, MAP_OK, MAP_SUPERSEDED };

// A keyframe's camera as CreateNewMapPoints reads it (:292-305, :337-349)
struct MapCam {
    float fx, fy, cx, cy, invfx, invfy;    // invfx = 1.0f / fx (KeyFrame's member)
    float Tcw[12];                         // rows of [Rcw | tcw]
    float Ow[3];
    float pad_[3];
};
// One feature as the pair tests read it: mvKeysUn[i].pt, mvLevelSigma2[octave], mvScaleFactors[octave]
struct MapFeat { float x, y, sigma2, scale; };

// :319-328: true = the neighbour is skipped
MAP_FN bool map_baseline_too_short(const float* Ow1, const float* Ow2, float medianDepthKF2)
{
    const float b0 = Ow2[0] - Ow1[0], b1 = Ow2[1] - Ow1[1], b2 = Ow2[2] - Ow1[2];
    const float baseline = (float)sqrt((double)b0 * b0 + (double)b1 * b1 + (double)b2 * b2);
    const float ratioBaselineDepth = baseline / medianDepthKF2;
    return (double)ratioBaselineDepth < 0.01;
}

// The epipolar line of (x1, y1) in the second image, l = x1' F12 = [a b c] (ORBmatcher.cpp:162-164)
MAP_FN void map_epipolar_line(const float* F12, float x1, float y1, float l[3])
{
    l[0] = x1 * F12[0] + y1 * F12[3] + F12[6];
    l[1] = x1 * F12[1] + y1 * F12[4] + F12[7];
    l[2] = x1 * F12[2] + y1 * F12[5] + F12[8];
}
// ORBmatcher.cpp:775-780 for a candidate whose distance already is <= TH_LOW: not near the epipole and on the epipolar line
MAP_FN bool map_candidate_ok(const float l[3], float ex, float ey, const MapFeat& f2)
{
    const float distex = ex - f2.x, distey = ey - f2.y;
    if (distex * distex + distey * distey < 100 * f2.scale) return false;
    const float num = l[0] * f2.x + l[1] * f2.y + l[2];
    const float den = l[0] * l[0] + l[1] * l[1];
    if (den == 0) return false;
    const float dsqr = num * num / den;
    return dsqr < 3.84 * f2.sigma2;
}

// cv::Mat row . x3Dt + t: the dot in double, the sum with the float in double, stored as float (:400, :404, :410 ...)
MAP_FN float map_row(const float* T, int r, const float X[3])
{
    const double d = (double)T[4 * r] * X[0] + (double)T[4 * r + 1] * X[1] + (double)T[4 * r + 2] * X[2];
    return (float)(d + (double)T[4 * r + 3]);
}
// ray = Rwc * xn with Rwc = Rcw^T (:366-367)
MAP_FN void map_ray(const float* T, const float xn[3], float ray[3])
{
#pragma unroll
    for (int r = 0; r < 3; r++) ray[r] = (float)((double)T[r] * xn[0] + (double)T[4 + r] * xn[1] + (double)T[8 + r] * xn[2]);
}
MAP_FN double map_norm3(const float v[3]) { return sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]); }

// The tests that follow the point (:399-448).  Split from map_pair so that the host check can feed any point.
MAP_FN int map_gates(const MapCam& c1, const MapCam& c2, const MapFeat& f1, const MapFeat& f2, float ratioFactor, const float X[3])
{
    const float z1 = map_row(c1.Tcw, 2, X);
    if (z1 <= 0) return MAP_BEHIND_1;
    const float z2 = map_row(c2.Tcw, 2, X);
    if (z2 <= 0) return MAP_BEHIND_2;
    {
        const float x1 = map_row(c1.Tcw, 0, X), y1 = map_row(c1.Tcw, 1, X);
        const float invz1 = (float)(1.0 / (double)z1);
        const float u1 = c1.fx * x1 * invz1 + c1.cx, v1 = c1.fy * y1 * invz1 + c1.cy;
        const float errX1 = u1 - f1.x, errY1 = v1 - f1.y;
        if ((errX1 * errX1 + errY1 * errY1) > 5.991 * f1.sigma2) return MAP_REPROJ_1;
    }
    {
        const float x2 = map_row(c2.Tcw, 0, X), y2 = map_row(c2.Tcw, 1, X);
        const float invz2 = (float)(1.0 / (double)z2);
        const float u2 = c2.fx * x2 * invz2 + c2.cx, v2 = c2.fy * y2 * invz2 + c2.cy;
        const float errX2 = u2 - f2.x, errY2 = v2 - f2.y;
        if ((errX2 * errX2 + errY2 * errY2) > 5.991 * f2.sigma2) return MAP_REPROJ_2;
    }
    const float n1[3] = { X[0] - c1.Ow[0], X[1] - c1.Ow[1], X[2] - c1.Ow[2] };
    const float n2[3] = { X[0] - c2.Ow[0], X[1] - c2.Ow[1], X[2] - c2.Ow[2] };
    const float dist1 = (float)map_norm3(n1), dist2 = (float)map_norm3(n2);
    if (dist1 == 0 || dist2 == 0) return MAP_ZERO_DIST;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = f1.scale / f2.scale;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return MAP_SCALE;
    return MAP_OK;
}

// One matched pair (:363-448): MAP_LOW_PARALLAX .. MAP_OK.  X is written (zero where no point was computed); *cosp = cosParallaxRays.
MAP_FN int map_pair(const MapCam& c1, const MapCam& c2, const MapFeat& f1, const MapFeat& f2, float ratioFactor, float X[3], float* cosp)
{
    X[0] = 0.0f; X[1] = 0.0f; X[2] = 0.0f;
    const float xn1[3] = { (f1.x - c1.cx) * c1.invfx, (f1.y - c1.cy) * c1.invfy, 1.0f };
    const float xn2[3] = { (f2.x - c2.cx) * c2.invfx, (f2.y - c2.cy) * c2.invfy, 1.0f };
    float ray1[3], ray2[3];
    map_ray(c1.Tcw, xn1, ray1); map_ray(c2.Tcw, xn2, ray2);
    const double dot = (double)ray1[0] * ray2[0] + (double)ray1[1] * ray2[1] + (double)ray1[2] * ray2[2];
    const float cosParallaxRays = (float)(dot / (map_norm3(ray1) * map_norm3(ray2)));
    *cosp = cosParallaxRays;
    const float cosParallaxStereo = cosParallaxRays + 1;
    if (!(cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (cosParallaxRays < 0.9998))) return MAP_LOW_PARALLAX;
    float A[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        A[0][c] = xn1[0] * c1.Tcw[8 + c] - c1.Tcw[c]; A[1][c] = xn1[1] * c1.Tcw[8 + c] - c1.Tcw[4 + c];
        A[2][c] = xn2[0] * c2.Tcw[8 + c] - c2.Tcw[c]; A[3][c] = xn2[1] * c2.Tcw[8 + c] - c2.Tcw[4 + c];
    }
    double M[4][4], V[4][4], x[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
            M[i][j] = (double)A[0][i] * A[0][j] + (double)A[1][i] * A[1][j] + (double)A[2][i] * A[2][j] + (double)A[3][i] * A[3][j];
    ini_jacobi<4>(M, V);
    ini_smallest<4>(M, V, x);
    const float x3 = (float)x[3];
    if (x3 == 0) return MAP_W_ZERO;
    X[0] = (float)x[0] / x3; X[1] = (float)x[1] / x3; X[2] = (float)x[2] / x3;                  // :391
    if (!std::isfinite(X[0]) || !std::isfinite(X[1]) || !std::isfinite(X[2])) return MAP_NONFINITE;
    return map_gates(c1, c2, f1, f2, ratioFactor, X);
}
