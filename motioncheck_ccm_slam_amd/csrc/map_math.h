// map_math.h -- the per-pair arithmetic of LocalMapping::CreateNewMapPoints (src/Mapping.cpp:312-448) and of the candidate test of
// ORBmatcher::SearchForTriangulation (ORBmatcher.cpp:768-784, CheckDistEpipolarLine :159-176).  Plain functions shared by the kernels
// (map_kernels.hip), the host (map_host.cpp) and the host check (tests/support/map_math_check.cpp).  Float storage and float
// arithmetic in the reference's operation order; the sums of cv::Mat products, dot and norm in double, stored as float; the null
// vector of the float 4x4 from the Jacobi of init_math.h in double on A^T A.  Built with -ffp-contract=off.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>
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

// ---- the geometry of one (current, neighbour) pair: the definitions behind ccm_map_pair_geometry and ccm_scene_median_depth
// (include/ccm_hot.h).  MAP_FN: the same text serves a device kernel that computes them from keyframe handles and the map-point table.

// A product of float 3x3 matrices as cv::gemm on CV_32F is read here: each entry summed in double over k ascending, stored as float.
// The products of two floats are exact in double, so a fused multiply-add would give the same sums.
MAP_FN void map_mul33(const float A[9], const float B[9], float C[9])
{
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            C[3 * i + j] = (float)((double)A[3 * i] * B[j] + (double)A[3 * i + 1] * B[3 + j] + (double)A[3 * i + 2] * B[6 + j]);
}
// K^-1 of K = [fx 0 cx; 0 fy cy; 0 0 1] in closed form: [1/fx 0 -cx/fx; 0 1/fy -cy/fy; 0 0 1], each entry one division in double
// stored as float: (float)(1.0 / fx) and (float)(-(double)cx / (double)fx) -- not the product form -cx * (1 / fx).  K^-T is its
// transpose, entry for entry.
MAP_FN void map_kinv(const float K[4], float Ki[9])
{
    Ki[0] = (float)(1.0 / (double)K[0]); Ki[1] = 0.0f; Ki[2] = (float)(-(double)K[2] / (double)K[0]);
    Ki[3] = 0.0f; Ki[4] = (float)(1.0 / (double)K[1]); Ki[5] = (float)(-(double)K[3] / (double)K[1]);
    Ki[6] = 0.0f; Ki[7] = 0.0f; Ki[8] = 1.0f;
}
// LocalMapping::ComputeF12 (src/Mapping.cpp:549-566) and the epipole of SearchForTriangulation (ORBmatcher.cpp:708-714).
//   R12 = R1w * R2w^T;  t12 = (-R1w * R2w^T) * t2w + t1w  (the product chain left to right, each product stored as float, the add in float)
//   F12 = ((K1^-T * [t12]x) * R12) * K2^-1
//   C2 = R2w * Ow1 + t2w;  invz = 1.0f / C2z;  ex = fx2 * C2x * invz + cx2, ey = fy2 * C2y * invz + cy2  (float)
// K = (fx, fy, cx, cy); Tcw = rows of [Rcw | tcw].
MAP_FN void map_pair_geometry(const float K1[4], const float* Tcw1, const float* Ow1, const float K2[4], const float* Tcw2, float F12[9], float epipole[2])
{
    float R1[9], R2t[9], nR1[9], R12[9], nR12[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { R1[3 * i + j] = Tcw1[4 * i + j]; nR1[3 * i + j] = -Tcw1[4 * i + j]; R2t[3 * i + j] = Tcw2[4 * j + i]; }
    map_mul33(R1, R2t, R12);
    map_mul33(nR1, R2t, nR12);
    float t12[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
        t12[i] = (float)((double)nR12[3 * i] * Tcw2[3] + (double)nR12[3 * i + 1] * Tcw2[7] + (double)nR12[3 * i + 2] * Tcw2[11]) + Tcw1[4 * i + 3];
    const float tx[9] = { 0.0f, -t12[2], t12[1], t12[2], 0.0f, -t12[0], -t12[1], t12[0], 0.0f };
    float K1i[9], K1it[9], K2i[9], A[9], B[9];
    map_kinv(K1, K1i); map_kinv(K2, K2i);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) K1it[3 * i + j] = K1i[3 * j + i];
    map_mul33(K1it, tx, A);
    map_mul33(A, R12, B);
    map_mul33(B, K2i, F12);
    float C2[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
        C2[i] = (float)((double)Tcw2[4 * i] * Ow1[0] + (double)Tcw2[4 * i + 1] * Ow1[1] + (double)Tcw2[4 * i + 2] * Ow1[2]) + Tcw2[4 * i + 3];
    const float invz = 1.0f / C2[2];
    epipole[0] = K2[0] * C2[0] * invz + K2[2];
    epipole[1] = K2[1] * C2[1] * invz + K2[3];
}

// KeyFrame::ComputeSceneMedianDepth(2) (src/KeyFrame.cpp:1241-1272) on the map-point table.  Feature i counts iff its id names a
// row of the table that is LIVE (bit 0 of the flags; a BAD row counts: the reference tests IsEmpty(), not isBad()) and its depth
// z = Rcw.row(2) . pos + tcw[2] (the dot in double, the add in double, stored as float) is finite.  The median is the depth of rank
// (m - 1) / 2 among the m counted ones, in the order of map_depth_key: ascending, -0.0f before +0.0f.
#define MAP_KEY_NONE 0xFFFFFFFFu           // above the key of every finite float (+inf has 0xFF800000)
MAP_FN float map_row(const float* T, int r, const float X[3]);      // below
MAP_FN uint32_t map_depth_key(float z)
{
    union { float f; uint32_t u; } v; v.f = z;
    return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
}
MAP_FN float map_key_depth(uint32_t k)
{
    union { float f; uint32_t u; } v;
    v.u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    return v.f;
}
// The key of feature i's depth, MAP_KEY_NONE when the feature does not count
MAP_FN uint32_t map_feature_depth_key(int32_t id, int capacity, const float* pos, const uint8_t* flags, const float* Tcw)
{
    if (id < 0 || id >= capacity || !(flags[id] & 1)) return MAP_KEY_NONE;
    const float z = map_row(Tcw, 2, pos + 3 * (size_t)id);
    return std::isfinite(z) ? map_depth_key(z) : MAP_KEY_NONE;
}

// The host form (ccm_scene_median_depth): the counted keys, then std::nth_element.  -> m, the number of counted depths; *median = 0 for m == 0.
inline int map_scene_median_depth(int n, const int32_t* mp_id, int capacity, const float* pos, const uint8_t* flags, const float* Tcw, float* median)
{
    std::vector<uint32_t> keys;
    keys.reserve((size_t)n);
    for (int i = 0; i < n; i++) {
        const uint32_t key = map_feature_depth_key(mp_id[i], capacity, pos, flags, Tcw);
        if (key != MAP_KEY_NONE) keys.push_back(key);
    }
    const int m = (int)keys.size();
    *median = 0.0f;
    if (m == 0) return 0;
    std::nth_element(keys.begin(), keys.begin() + (m - 1) / 2, keys.end());
    *median = map_key_depth(keys[(size_t)(m - 1) / 2]);
    return m;
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
