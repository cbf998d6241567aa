// init_math.h -- the per-hypothesis and per-match arithmetic of cslam::Initializer (src/Initializer.cpp): the rows of ComputeH21 /
// ComputeF21 (:222-299), what follows their null vector (:155-157, :292-298, :208), one term of CheckHomography / CheckFundamental
// (:333-381, :409-461) and one match of CheckRT (:826-890).  Plain functions shared by the kernels (init_kernels.hip) and the host
// (init_host.cpp).  Float storage and float per-match arithmetic in the reference's operation order; eigenproblems in double.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define INI_FN __host__ __device__ inline
#else
#define INI_FN inline
#endif

// The Jacobi rotation that zeroes a[p][q] of a symmetric matrix: a' = J^T a J with J = [c s; -s c] on (p, q).
INI_FN void ini_rotation(double app, double aqq, double apq, double* c, double* s)
{
    *c = 1.0; *s = 0.0;
    if (apq != 0.0) {
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        *c = 1.0 / sqrt(t * t + 1.0); *s = t * *c;
    }
}
// true: the entry is already negligible against both diagonal entries and the rotation is skipped
INI_FN bool ini_negligible(double app, double aqq, double apq) { return fabs(apq) <= 1e-17 * sqrt(fabs(app * aqq)); }

// The rotation (p, q) of the 9x9 Jacobi in two halves, each written for the owner k of one row / one column so that 9 lanes can share
// the matrix: first a J and V J on row k, then -- after every row is done -- J^T (a J) on column k.  M and V are row-major 9x9.
INI_FN void ini_jacobi9_row(double* M, double* V, int k, int p, int q, double c, double s)
{
    const double akp = M[9 * k + p], akq = M[9 * k + q];
    M[9 * k + p] = c * akp - s * akq; M[9 * k + q] = s * akp + c * akq;
    const double vkp = V[9 * k + p], vkq = V[9 * k + q];
    V[9 * k + p] = c * vkp - s * vkq; V[9 * k + q] = s * vkp + c * vkq;
}
INI_FN void ini_jacobi9_col(double* M, int k, int p, int q, double c, double s)
{
    const double apk = M[9 * p + k], aqk = M[9 * q + k];
    M[9 * p + k] = c * apk - s * aqk; M[9 * q + k] = s * apk + c * aqk;
}
// column of V that belongs to the smallest diagonal entry of M (the first of equal ones)
INI_FN int ini_jacobi9_smallest(const double* M)
{
    int jmin = 0; double best = M[0];
#pragma unroll
    for (int j = 1; j < 9; j++) { const double d = M[10 * j]; if (d < best) { best = d; jmin = j; } }
    return jmin;
}

// Eigen-decomposition of the symmetric N x N a (N = 3, 4; cyclic Jacobi, fixed sweeps, fully unrolled: registers on the device).
// On return the diagonal of a holds the eigenvalues and the columns of v the eigenvectors.
template <int N> INI_FN void ini_jacobi(double a[N][N], double v[N][N])
{
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 8; sweep++) {
#pragma unroll
        for (int p = 0; p < N - 1; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                double c, s;
                ini_rotation(a[p][p], a[q][q], a[p][q], &c, &s);
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq;
                }
            }
    }
}
// eigenvector of the smallest eigenvalue (the last row of vt of cv::SVDecomp)
template <int N> INI_FN void ini_smallest(double a[N][N], double v[N][N], double x[N])
{
    double best = a[0][0];
#pragma unroll
    for (int k = 0; k < N; k++) x[k] = v[k][0];
#pragma unroll
    for (int j = 1; j < N; j++) {
        const bool lo = a[j][j] < best;
        best = lo ? a[j][j] : best;
#pragma unroll
        for (int k = 0; k < N; k++) x[k] = lo ? v[k][j] : x[k];
    }
}

// C = A * B for 3x3 float matrices, row-major; sums in double, stored as float (as cv::gemm does for CV_32F)
INI_FN void ini_mul3(const float* A, const float* B, float* C)
{
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            C[3 * r + c] = (float)((double)A[3 * r] * B[c] + (double)A[3 * r + 1] * B[3 + c] + (double)A[3 * r + 2] * B[6 + c]);
}
// T of Normalize (:786-790) from sX, sY, meanX, meanY
INI_FN void ini_T(const float n[4], float T[9])
{
    T[0] = n[0]; T[1] = 0; T[2] = -n[2] * n[0]; T[3] = 0; T[4] = n[1]; T[5] = -n[3] * n[1]; T[6] = 0; T[7] = 0; T[8] = 1;
}
INI_FN void ini_inv3(const float* A, float* B)
{
    const double a = A[0], b = A[1], c = A[2], d = A[3], e = A[4], f = A[5], g = A[6], h = A[7], i = A[8];
    const double C0 = e * i - f * h, C1 = f * g - d * i, C2 = d * h - e * g;
    const double inv = 1.0 / (a * C0 + b * C1 + c * C2);
    B[0] = (float)(C0 * inv); B[1] = (float)((c * h - b * i) * inv); B[2] = (float)((b * f - c * e) * inv);
    B[3] = (float)(C1 * inv); B[4] = (float)((a * i - c * g) * inv); B[5] = (float)((c * d - a * f) * inv);
    B[6] = (float)(C2 * inv); B[7] = (float)((b * g - a * h) * inv); B[8] = (float)((a * e - b * d) * inv);
}

// Row r (0..15) of the 16 x 9 matrix of ComputeH21 (:235-253) for the normalised point pair (u1, v1) -> (u2, v2) of r / 2
INI_FN void ini_row_h(int r, float u1, float v1, float u2, float v2, float a[9])
{
    if ((r & 1) == 0) { a[0] = 0; a[1] = 0; a[2] = 0; a[3] = -u1; a[4] = -v1; a[5] = -1; a[6] = v2 * u1; a[7] = v2 * v1; a[8] = v2; }
    else              { a[0] = u1; a[1] = v1; a[2] = 1; a[3] = 0; a[4] = 0; a[5] = 0; a[6] = -u2 * u1; a[7] = -u2 * v1; a[8] = -u2; }
}
// Row of the 8 x 9 matrix of ComputeF21 (:277-285)
INI_FN void ini_row_f(float u1, float v1, float u2, float v2, float a[9])
{
    a[0] = u2 * u1; a[1] = u2 * v1; a[2] = u2; a[3] = v2 * u1; a[4] = v2 * v1; a[5] = v2; a[6] = u1; a[7] = v1; a[8] = 1;
}

// :155-157: Hn = the null vector as a float 3x3, H21i = T2inv * Hn * T1, H12i = H21i^-1
INI_FN void ini_finish_h(const double x[9], const float n1[4], const float n2[4], float H21[9], float H12[9])
{
    float Hn[9], T1[9], P[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Hn[k] = (float)x[k];
    ini_T(n1, T1);
    const float T2inv[9] = { 1.0f / n2[0], 0, n2[2], 0, 1.0f / n2[1], n2[3], 0, 0, 1 };
    ini_mul3(T2inv, Hn, P); ini_mul3(P, T1, H21);
    ini_inv3(H21, H12);
}
// :292-298 and :208: Fpre = the null vector as a float 3x3, its smallest singular value set to zero (Fpre (I - v3 v3^T) with v3 the
// eigenvector of the smallest eigenvalue of Fpre^T Fpre = u diag(w1, w2, 0) vt), F21i = T2^T * Fn * T1
INI_FN void ini_finish_f(const double x[9], const float n1[4], const float n2[4], float F21[9])
{
    float Fp[9], Fn[9], T1[9], T2[9], T2t[9], P[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Fp[k] = (float)x[k];
    double B[3][3], V[3][3], v3[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) B[i][j] = (double)Fp[i] * Fp[j] + (double)Fp[3 + i] * Fp[3 + j] + (double)Fp[6 + i] * Fp[6 + j];
    ini_jacobi<3>(B, V);
    ini_smallest<3>(B, V, v3);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double fv = (double)Fp[3 * r] * v3[0] + (double)Fp[3 * r + 1] * v3[1] + (double)Fp[3 * r + 2] * v3[2];
#pragma unroll
        for (int c = 0; c < 3; c++) Fn[3 * r + c] = (float)((double)Fp[3 * r + c] - fv * v3[c]);
    }
    ini_T(n1, T1); ini_T(n2, T2);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) T2t[3 * r + c] = T2[3 * c + r];
    ini_mul3(T2t, Fn, P); ini_mul3(P, T1, F21);
}

// One match of CheckHomography (:335-380): *in = bIn, the return value is what the two `score +=` add (0 for a failed direction).
INI_FN void ini_check_h(const float* H21, const float* H12, float u1, float v1, float u2, float v2, float invSigmaSquare, bool* in,
                        float* s1, float* s2)
{
    const float th = 5.991f;
    const float w2in1inv = 1.0f / (H12[6] * u2 + H12[7] * v2 + H12[8]);
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    const float w1in2inv = 1.0f / (H21[6] * u1 + H21[7] * v1 + H21[8]);
    const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
    const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    const bool out1 = chiSquare1 > th, out2 = chiSquare2 > th;
    *in = !out1 && !out2;
    *s1 = out1 ? 0.0f : th - chiSquare1;
    *s2 = out2 ? 0.0f : th - chiSquare2;
}
// One match of CheckFundamental (:411-460)
INI_FN void ini_check_f(const float* F, float u1, float v1, float u2, float v2, float invSigmaSquare, bool* in, float* s1, float* s2)
{
    const float th = 3.841f, thScore = 5.991f;
    const float a2 = F[0] * u1 + F[1] * v1 + F[2];
    const float b2 = F[3] * u1 + F[4] * v1 + F[5];
    const float c2 = F[6] * u1 + F[7] * v1 + F[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    const float a1 = F[0] * u2 + F[3] * v2 + F[6];
    const float b1 = F[1] * u2 + F[4] * v2 + F[7];
    const float c1 = F[2] * u2 + F[5] * v2 + F[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    const bool out1 = chiSquare1 > th, out2 = chiSquare2 > th;
    *in = !out1 && !out2;
    *s1 = out1 ? 0.0f : thScore - chiSquare1;
    *s2 = out2 ? 0.0f : thScore - chiSquare2;
}

// One inlier match of CheckRT (:831-889) for the motion (R, t): Triangulate (:730-743) with the null vector of the float 4x4 from a
// Jacobi in double on A^T A, then the tests in order.  Returns bit 0 = the match is counted in nGood (cosParallax is pushed and vP3D
// written), bit 1 = vbGood (cosParallax < 0.99998).  X and *cosp are written whenever bit 0 is set.
INI_FN int ini_check_rt(const float K[4], const float R[9], const float t[3], const float O2[3], const float P2[12], float th2, float u1,
                        float v1, float u2, float v2, float X[3], float* cosp)
{
    const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    const float P1[12] = { fx, 0, cx, 0, 0, fy, cy, 0, 0, 0, 1, 0 };
    float A[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        A[0][c] = u1 * P1[8 + c] - P1[c]; A[1][c] = v1 * P1[8 + c] - P1[4 + c];
        A[2][c] = u2 * P2[8 + c] - P2[c]; A[3][c] = v2 * P2[8 + c] - P2[4 + c];
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
    const float p0 = (float)x[0] / x3, p1 = (float)x[1] / x3, p2 = (float)x[2] / x3;          // :742
    X[0] = p0; X[1] = p1; X[2] = p2; *cosp = 0.0f;
    if (!std::isfinite(p0) || !std::isfinite(p1) || !std::isfinite(p2)) return 0;             // :837
    const float dist1 = (float)sqrt((double)p0 * p0 + (double)p1 * p1 + (double)p2 * p2);     // cv::norm sums in double
    const float n0 = p0 - O2[0], n1 = p1 - O2[1], n2 = p2 - O2[2];
    const float dist2 = (float)sqrt((double)n0 * n0 + (double)n1 * n1 + (double)n2 * n2);
    const float cosParallax = (float)(((double)p0 * n0 + (double)p1 * n1 + (double)p2 * n2) / (double)(dist1 * dist2));       // :850
    *cosp = cosParallax;
    const bool low = (double)cosParallax < 0.99998;
    if (p2 <= 0 && low) return 0;                                                              // :853
    const float q0 = (float)((double)R[0] * p0 + (double)R[1] * p1 + (double)R[2] * p2) + t[0];                               // :857
    const float q1 = (float)((double)R[3] * p0 + (double)R[4] * p1 + (double)R[5] * p2) + t[1];
    const float q2 = (float)((double)R[6] * p0 + (double)R[7] * p1 + (double)R[8] * p2) + t[2];
    if (q2 <= 0 && low) return 0;                                                              // :859
    const float invZ1 = 1.0f / p2;
    const float im1x = fx * p0 * invZ1 + cx, im1y = fy * p1 * invZ1 + cy;
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (squareError1 > th2) return 0;                                                          // :870
    const float invZ2 = 1.0f / q2;
    const float im2x = fx * q0 * invZ2 + cx, im2y = fy * q1 * invZ2 + cy;
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (squareError2 > th2) return 0;                                                          // :881
    return low ? 3 : 1;                                                                        // :884-889
}
