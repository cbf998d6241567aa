// sim3_ransac_math.h -- one hypothesis of Sim3Solver::iterate (src/Sim3Solver.cpp:146-165): the sampling map, Horn's closed
// form (ComputeSim3, :210-321) and the two reprojection errors of CheckInliers (:324-348).  Plain functions shared by the kernel
// (sim3_ransac_kernels.hip) and by host-side checks; float storage as in the reference, the 4x4 eigenproblem in double.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define S3R_FN __host__ __device__ inline
#else
#define S3R_FN inline
#endif

struct S3rXf { float T12[12], T21[12]; };          // rows 0..2 of mT12i / mT21i: [sR | t]

// :146-161 without the vector: vAvailableIndices starts as 0..n-1, draw i picks position r[i] of what is left and the last element
// takes that position (vAvailableIndices[randi] = back, :159).  r[i] in [0, n-1-i], n >= 3.
S3R_FN void s3r_sample(int n, const int r[3], int idx[3])
{
    idx[0] = r[0];                                                         // untouched list
    idx[1] = r[1] == r[0] ? n - 1 : r[1];                                  // position r0 now holds n-1
    const int back1 = r[0] == n - 2 ? n - 1 : n - 2;                       // last element of the list of n-1
    idx[2] = r[2] == r[1] ? back1 : (r[2] == r[0] ? n - 1 : r[2]);
}

// Eigenvector of the largest eigenvalue of the symmetric 4x4 a (cyclic Jacobi, a fixed number of sweeps: every lane of a wave does
// the same work and a hypothesis' result does not depend on its neighbours').  q = (w, x, y, z), unit length.
S3R_FN void s3r_top_eigenvector(double a[4][4], double q[4])
{
    double v[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 10; sweep++) {
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int r = p + 1; r < 4; r++) {
                const double apr = a[p][r];
                double c = 1.0, s = 0.0;
                if (apr != 0.0) {
                    const double theta = (a[r][r] - a[p][p]) / (2.0 * apr);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0); s = t * c;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double akp = a[k][p], akr = a[k][r];
                    a[k][p] = c * akp - s * akr; a[k][r] = s * akp + c * akr;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double apk = a[p][k], ark = a[r][k];
                    a[p][k] = c * apk - s * ark; a[r][k] = s * apk + c * ark;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double vkp = v[k][p], vkr = v[k][r];
                    v[k][p] = c * vkp - s * vkr; v[k][r] = s * vkp + c * vkr;
                }
            }
    }
    double best = a[0][0];
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = v[k][0];
#pragma unroll
    for (int j = 1; j < 4; j++) {
        const bool up = a[j][j] > best;
        best = up ? a[j][j] : best;
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = up ? v[k][j] : q[k];
    }
    const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] /= nrm;
}

// ComputeSim3(P1, P2) (:210-321): P1[i], P2[i] = the i-th sampled point (a column of P3Dc1i / P3Dc2i).  Rts = R12 (row-major 9),
// t12 (3), s12.  The rotation comes from the unit quaternion itself; it is the Rodrigues matrix of the angle-axis vector the
// reference forms at :262-268, for either sign of the eigenvector, and is defined at zero rotation.
S3R_FN void s3r_horn(const float P1[3][3], const float P2[3][3], bool fix_scale, float Rts[13], S3rXf* X)
{
    float O1[3], O2[3], Pr1[3][3], Pr2[3][3];                              // ComputeCentroid (:199-208)
#pragma unroll
    for (int d = 0; d < 3; d++) {
        O1[d] = (P1[0][d] + P1[1][d] + P1[2][d]) / 3.0f;
        O2[d] = (P2[0][d] + P2[1][d] + P2[2][d]) / 3.0f;
#pragma unroll
        for (int i = 0; i < 3; i++) { Pr1[i][d] = P1[i][d] - O1[d]; Pr2[i][d] = P2[i][d] - O2[d]; }
    }
    float M[3][3];                                                         // M = Pr2 * Pr1^T (:227)
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) M[r][c] = Pr2[0][r] * Pr1[0][c] + Pr2[1][r] * Pr1[1][c] + Pr2[2][r] * Pr1[2][c];
    // :231-249: the entries are formed in double and stored in a float matrix
    const float N11 = (float)((double)M[0][0] + M[1][1] + M[2][2]), N12 = (float)((double)M[1][2] - M[2][1]);
    const float N13 = (float)((double)M[2][0] - M[0][2]), N14 = (float)((double)M[0][1] - M[1][0]);
    const float N22 = (float)((double)M[0][0] - M[1][1] - M[2][2]), N23 = (float)((double)M[0][1] + M[1][0]);
    const float N24 = (float)((double)M[2][0] + M[0][2]), N33 = (float)(-(double)M[0][0] + M[1][1] - M[2][2]);
    const float N34 = (float)((double)M[1][2] + M[2][1]), N44 = (float)(-(double)M[0][0] - M[1][1] + M[2][2]);
    double A[4][4] = { { N11, N12, N13, N14 }, { N12, N22, N23, N24 }, { N13, N23, N33, N34 }, { N14, N24, N34, N44 } };
    double q[4];
    s3r_top_eigenvector(A, q);                                             // cv::eigen, row 0 (:256)
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    float R[9] = { (float)(1 - 2 * (y * y + z * z)), (float)(2 * (x * y - z * w)), (float)(2 * (x * z + y * w)),
                   (float)(2 * (x * y + z * w)), (float)(1 - 2 * (x * x + z * z)), (float)(2 * (y * z - x * w)),
                   (float)(2 * (x * z - y * w)), (float)(2 * (y * z + x * w)), (float)(1 - 2 * (x * x + y * y)) };
    float s = 1.0f;
    if (!fix_scale) {                                                      // :276-293: both sums in double over float products
        double nom = 0, den = 0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int d = 0; d < 3; d++) {
                const float p3 = R[3 * d] * Pr2[i][0] + R[3 * d + 1] * Pr2[i][1] + R[3 * d + 2] * Pr2[i][2];   // P3 = R * Pr2 (:272)
                nom += (double)Pr1[i][d] * (double)p3;
                den += (double)(p3 * p3);
            }
        s = (float)(nom / den);
    }
    float t[3];                                                            // t = O1 - s R O2 (:300)
#pragma unroll
    for (int d = 0; d < 3; d++) t[d] = O1[d] - (s * R[3 * d] * O2[0] + s * R[3 * d + 1] * O2[1] + s * R[3 * d + 2] * O2[2]);
#pragma unroll
    for (int k = 0; k < 9; k++) Rts[k] = R[k];
    Rts[9] = t[0]; Rts[10] = t[1]; Rts[11] = t[2]; Rts[12] = s;
    const double inv_s = 1.0 / (double)s;                                  // :316
    float Ri[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            X->T12[4 * r + c] = s * R[3 * r + c];                          // :307
            Ri[3 * r + c] = (float)(inv_s * (double)R[3 * c + r]);
            X->T21[4 * r + c] = Ri[3 * r + c];
        }
#pragma unroll
    for (int r = 0; r < 3; r++) {
        X->T12[4 * r + 3] = t[r];
        X->T21[4 * r + 3] = -(Ri[3 * r] * t[0] + Ri[3 * r + 1] * t[1] + Ri[3 * r + 2] * t[2]);   // tinv = -sRinv * t (:319)
    }
}

// FromCameraToImage / Project (:366-407): pinhole projection of T * X (T = rows of [R | t], or nullptr for the identity)
S3R_FN void s3r_project(const float* T, const float K[4], float x, float y, float z, float* u, float* v)
{
    float px = x, py = y, pz = z;
    if (T) {
        px = T[0] * x + T[1] * y + T[2] * z + T[3];
        py = T[4] * x + T[5] * y + T[6] * z + T[7];
        pz = T[8] * x + T[9] * y + T[10] * z + T[11];
    }
    const float invz = 1.0f / pz;
    *u = K[0] * (px * invz) + K[2];
    *v = K[1] * (py * invz) + K[3];
}
