// pnp_math.h -- the arithmetic of cslam::PnPsolver (src/PnPSolver.cpp): EPnP compute_pose (:468-516) for n >= 4 correspondences in
// double, and one correspondence of CheckInliers (:299-330) in the reference's mixed float / double typing.  Plain functions shared
// by the kernels (pnp_kernels.hip) and the host (pnp_host.cpp: ccm_pnp_compute_pose is this header through the host compiler).
//
// compute_pose is cut where its sums over the n correspondences are, so that one caller can run it serially (pnp_compute_pose
// below: one hypothesis per lane, or the host) and another can reduce the sums across lanes and run only the small algebra in
// between (k_pnp_refine).  What the reference takes from OpenCV is restated with Jacobi iterations: the 3x3 and 12x12 symmetric
// eigenproblems two-sided, the 3x3 SVD of estimate_R_and_t and the 6xk least squares of find_betas_approx_* one-sided (Hestenes),
// which works on the matrix itself and keeps its conditioning.  The basis of the null space of M^T M that comes out of a Jacobi
// iteration is as arbitrary as the one OpenCV returns (DESIGN.md "PnPsolver"); everything behind (control points, basis) is a
// well-conditioned function of that pair and is held to a float64 restatement fed with it.
#pragma once
#include <cmath>
#include "init_math.h"

#define PNP_FN INI_FN
#define PNP_DETAIL 68          // doubles per row of the detail tap: cws 12, basis 48, betas 4, rep_error 3, which 1
#define PNP_AXIS_EPS 1e-7      // a PCA axis shorter than this times the longest counts as vanishing (pseudo-inverse, as cvInvert(CV_SVD))
#define PNP_RANK_EPS 1e-12     // singular values below this times the largest are dropped by the minimum-norm least squares

// ---------------------------------------------------------------------------------------------------------------- small pieces
PNP_FN double pnp_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PNP_FN double pnp_dist2(const double* a, const double* b)
{
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// One-sided Jacobi: rotates the columns of A (R x C) until they are orthogonal, A_in V = A_out.  The columns of A_out are sigma_j u_j.
template <int R, int C> PNP_FN void pnp_onesided(double A[R][C], double V[C][C])
{
#pragma unroll
    for (int i = 0; i < C; i++)
#pragma unroll
        for (int j = 0; j < C; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 12; sweep++) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < C - 1; p++)
#pragma unroll
            for (int q = p + 1; q < C; q++) {
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int k = 0; k < R; k++) { al += A[k][p] * A[k][p]; be += A[k][q] * A[k][q]; ga += A[k][p] * A[k][q]; }
                if (fabs(ga) <= 1e-17 * sqrt(al * be)) continue;
                rotated = true;
                double c, s;
                ini_rotation(al, be, ga, &c, &s);
#pragma unroll
                for (int k = 0; k < R; k++) { const double x = A[k][p], y = A[k][q]; A[k][p] = c * x - s * y; A[k][q] = s * x + c * y; }
#pragma unroll
                for (int k = 0; k < C; k++) { const double x = V[k][p], y = V[k][q]; V[k][p] = c * x - s * y; V[k][q] = s * x + c * y; }
            }
        if (!rotated) break;
    }
}

// Minimum-norm least-squares solution of the 6 x C system A x = b (cvSolve(CV_SVD) at :672, :703, :737).  A is destroyed.
template <int C> PNP_FN void pnp_lstsq6(double A[6][C], const double b[6], double x[C])
{
    double V[C][C], s2[C], smax = 0.0;
    pnp_onesided<6, C>(A, V);
#pragma unroll
    for (int j = 0; j < C; j++) {
        s2[j] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) s2[j] += A[k][j] * A[k][j];
        smax = s2[j] > smax ? s2[j] : smax;
    }
#pragma unroll
    for (int i = 0; i < C; i++) x[i] = 0.0;
#pragma unroll
    for (int j = 0; j < C; j++) {
        double w = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) w += A[k][j] * b[k];
        w = s2[j] > PNP_RANK_EPS * PNP_RANK_EPS * smax ? w / s2[j] : 0.0;
#pragma unroll
        for (int i = 0; i < C; i++) x[i] += V[i][j] * w;
    }
}

// ------------------------------------------------------------------------------------------------- choose_control_points :366-400
// c0 = the centroid, cov = sum (p - c0)(p - c0)^T as xx xy xz yy yz zz.  cws[0] = c0, cws[1 + j] = c0 + sqrt(lambda_j / n) axis_j with
// lambda descending as cvSVD orders them.  ci = the pseudo-inverse of [cws[1]-c0 | cws[2]-c0 | cws[3]-c0] (:404-412), row j =
// axis_j / sqrt(lambda_j / n), or zero for a vanishing axis.
PNP_FN void pnp_cswap(double* lam, double ax[3][3], int i, int j)
{
    if (lam[i] < lam[j]) {
        const double l = lam[i]; lam[i] = lam[j]; lam[j] = l;
#pragma unroll
        for (int k = 0; k < 3; k++) { const double t = ax[i][k]; ax[i][k] = ax[j][k]; ax[j][k] = t; }
    }
}
PNP_FN void pnp_control_points(int n, const double c0[3], const double cov[6], double cws[4][3], double ci[3][3])
{
    double a[3][3] = { { cov[0], cov[1], cov[2] }, { cov[1], cov[3], cov[4] }, { cov[2], cov[4], cov[5] } }, v[3][3];
    ini_jacobi<3>(a, v);
    double lam[3] = { a[0][0], a[1][1], a[2][2] }, ax[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int k = 0; k < 3; k++) ax[j][k] = v[k][j];
    pnp_cswap(lam, ax, 0, 1); pnp_cswap(lam, ax, 1, 2); pnp_cswap(lam, ax, 0, 1);
    double kk[3];
#pragma unroll
    for (int j = 0; j < 3; j++) kk[j] = sqrt((lam[j] > 0.0 ? lam[j] : 0.0) / n);
#pragma unroll
    for (int k = 0; k < 3; k++) cws[0][k] = c0[k];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            cws[1 + j][k] = c0[k] + kk[j] * ax[j][k];
            ci[j][k] = kk[j] > PNP_AXIS_EPS * kk[0] ? ax[j][k] / kk[j] : 0.0;
        }
}
// compute_barycentric_coordinates :414-424 for one point
PNP_FN void pnp_alphas(const double ci[3][3], const double c0[3], const double p[3], double a[4])
{
    const double d[3] = { p[0] - c0[0], p[1] - c0[1], p[2] - c0[2] };
#pragma unroll
    for (int j = 0; j < 3; j++) a[1 + j] = ci[j][0] * d[0] + ci[j][1] * d[1] + ci[j][2] * d[2];
    a[0] = 1.0 - a[1] - a[2] - a[3];
}
// fill_M :427-442: the two rows of one correspondence.  K = fu, fv, uc, vc.
PNP_FN void pnp_rows_M(const double a[4], const double uv[2], const double K[4], double m1[12], double m2[12])
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        m1[3 * i] = a[i] * K[0]; m1[3 * i + 1] = 0.0;         m1[3 * i + 2] = a[i] * (K[2] - uv[0]);
        m2[3 * i] = 0.0;         m2[3 * i + 1] = a[i] * K[1]; m2[3 * i + 2] = a[i] * (K[3] - uv[1]);
    }
}

// ------------------------------------------------------------------------------------- M^T M and its eigenvectors (:483-484)
// A 12x12 matrix behind an accessor, so that the device can keep it in LDS ([element][lane] for one hypothesis per lane).
struct PnpMatHost {
    double m[144];
    PNP_FN double& operator()(int i, int j) { return m[12 * i + j]; }
};
struct PnpMatStrided {
    double* base; int stride;
    PNP_FN double& operator()(int i, int j) { return base[(12 * i + j) * stride]; }
};

// The rotation (p, q) of pnp_jacobi12: columns p and q of A and V, then rows p and q of A.  Every load of a phase comes before its
// first store, so that the loads of a lane are in flight together (the matrices live behind pointers the compiler must take to alias).
template <class Mat> PNP_FN void pnp_rotate12(Mat& A, Mat& V, const int p, const int q, const double c, const double s)
{
    double xp[12], xq[12], yp[12], yq[12];
#pragma unroll 12
    for (int k = 0; k < 12; k++) { xp[k] = A(k, p); xq[k] = A(k, q); yp[k] = V(k, p); yq[k] = V(k, q); }
#pragma unroll 12
    for (int k = 0; k < 12; k++) {
        A(k, p) = c * xp[k] - s * xq[k]; A(k, q) = s * xp[k] + c * xq[k];
        V(k, p) = c * yp[k] - s * yq[k]; V(k, q) = s * yp[k] + c * yq[k];
    }
#pragma unroll 12
    for (int k = 0; k < 12; k++) { xp[k] = A(p, k); xq[k] = A(q, k); }
#pragma unroll 12
    for (int k = 0; k < 12; k++) { A(p, k) = c * xp[k] - s * xq[k]; A(q, k) = s * xp[k] + c * xq[k]; }
}

// Cyclic Jacobi on the symmetric 12x12 A: on return the diagonal of A holds the eigenvalues and the columns of V the eigenvectors.
// An entry is skipped once it is negligible against both diagonal entries or against the matrix (floor: the entries of the null
// space of a minimal set never become small against their own diagonal).  Ends after the first sweep without a rotation.
template <class Mat> PNP_FN void pnp_jacobi12(Mat& A, Mat& V)
{
    double tr = 0.0;
    for (int i = 0; i < 12; i++) {
        tr += fabs(A(i, i));
        for (int j = 0; j < 12; j++) V(i, j) = i == j ? 1.0 : 0.0;
    }
    const double floor_ = 1e-16 * tr;
    for (int sweep = 0; sweep < 16; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 11; p++)
            for (int q = p + 1; q < 12; q++) {
                const double app = A(p, p), aqq = A(q, q), apq = A(p, q);
                if (fabs(apq) <= floor_ || ini_negligible(app, aqq, apq)) continue;
                rotated = true;
                double c, s;
                ini_rotation(app, aqq, apq, &c, &s);
                pnp_rotate12(A, V, p, q, c, s);
            }
        if (!rotated) break;
    }
}
// v[0..3] = ut rows 11..8 (:755-758): the eigenvectors of the four smallest eigenvalues, smallest first (the first of equal ones).
template <class Mat> PNP_FN void pnp_basis(Mat& A, Mat& V, double basis[4][12])
{
    unsigned used = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int best = -1; double lo = 0.0;
        for (int j = 0; j < 12; j++) {
            const double d = A(j, j);
            if (!(used >> j & 1) && (best < 0 || d < lo)) { best = j; lo = d; }
        }
        used |= 1u << best;
#pragma unroll
        for (int k = 0; k < 12; k++) basis[r][k] = V(k, best);
    }
}

// --------------------------------------------------------------------------------- the betas: :487-507 without compute_R_and_t
// compute_L_6x10 :751-791 and compute_rho :793-801; the pairs (a, b) of control points in the order of :763-774
PNP_FN void pnp_L_rho(const double v[4][12], const double cws[4][3], double L[6][10], double rho[6])
{
    const int pa[6] = { 0, 0, 0, 1, 1, 2 }, pb[6] = { 1, 2, 3, 2, 3, 3 };
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double dv[4][3];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) dv[i][k] = v[i][3 * pa[j] + k] - v[i][3 * pb[j] + k];
        L[j][0] = pnp_dot3(dv[0], dv[0]);
        L[j][1] = 2.0 * pnp_dot3(dv[0], dv[1]);
        L[j][2] = pnp_dot3(dv[1], dv[1]);
        L[j][3] = 2.0 * pnp_dot3(dv[0], dv[2]);
        L[j][4] = 2.0 * pnp_dot3(dv[1], dv[2]);
        L[j][5] = pnp_dot3(dv[2], dv[2]);
        L[j][6] = 2.0 * pnp_dot3(dv[0], dv[3]);
        L[j][7] = 2.0 * pnp_dot3(dv[1], dv[3]);
        L[j][8] = 2.0 * pnp_dot3(dv[2], dv[3]);
        L[j][9] = pnp_dot3(dv[3], dv[3]);
        rho[j] = pnp_dist2(cws[pa[j]], cws[pb[j]]);
    }
}
// find_betas_approx_1 :658-685: unknowns B11 B12 B13 B14
PNP_FN void pnp_betas_1(const double L[6][10], const double rho[6], double betas[4])
{
    double A[6][4], b[4];
#pragma unroll
    for (int i = 0; i < 6; i++) { A[i][0] = L[i][0]; A[i][1] = L[i][1]; A[i][2] = L[i][3]; A[i][3] = L[i][6]; }
    pnp_lstsq6<4>(A, rho, b);
    const double sg = b[0] < 0 ? -1.0 : 1.0;
    betas[0] = sqrt(sg * b[0]);
    betas[1] = sg * b[1] / betas[0]; betas[2] = sg * b[2] / betas[0]; betas[3] = sg * b[3] / betas[0];
}
// the common part of :705-713 and :739-746
PNP_FN void pnp_betas_01(double b0, double b1, double b2, double betas[4])
{
    if (b0 < 0) { betas[0] = sqrt(-b0); betas[1] = b2 < 0 ? sqrt(-b2) : 0.0; }
    else        { betas[0] = sqrt(b0);  betas[1] = b2 > 0 ? sqrt(b2) : 0.0; }
    if (b1 < 0) betas[0] = -betas[0];
}
// find_betas_approx_2 :690-717: unknowns B11 B12 B22
PNP_FN void pnp_betas_2(const double L[6][10], const double rho[6], double betas[4])
{
    double A[6][3], b[3];
#pragma unroll
    for (int i = 0; i < 6; i++) { A[i][0] = L[i][0]; A[i][1] = L[i][1]; A[i][2] = L[i][2]; }
    pnp_lstsq6<3>(A, rho, b);
    pnp_betas_01(b[0], b[1], b[2], betas);
    betas[2] = 0.0; betas[3] = 0.0;
}
// find_betas_approx_3 :722-749: unknowns B11 B12 B22 B13 B23
PNP_FN void pnp_betas_3(const double L[6][10], const double rho[6], double betas[4])
{
    double A[6][5], b[5];
#pragma unroll
    for (int i = 0; i < 6; i++) { A[i][0] = L[i][0]; A[i][1] = L[i][1]; A[i][2] = L[i][2]; A[i][3] = L[i][3]; A[i][4] = L[i][4]; }
    pnp_lstsq6<5>(A, rho, b);
    pnp_betas_01(b[0], b[1], b[2], betas);
    betas[2] = b[3] / betas[0]; betas[3] = 0.0;
}
// qr_solve :851-941 for the 6x4 system of gauss_newton, in the reference's operation order: Householder columns scaled by eta, which
// the reference takes over rows k .. nr-2 (its scan reads each entry before it advances, so the last row never enters), b <- Q^T b,
// back substitution.  eta == 0: the reference returns with X stale (uninitialised on the first step); here the step is zero.
PNP_FN void pnp_qr_solve(double A[6][4], double b[6], double x[4])
{
    double A1[4], A2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double eta = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 5; i++) { const double e = fabs(A[i][k]); if (eta < e) eta = e; }
        if (eta == 0) { x[0] = x[1] = x[2] = x[3] = 0.0; return; }
        const double inv_eta = 1. / eta;
        double sum = 0.0;
#pragma unroll
        for (int i = k; i < 6; i++) { A[i][k] *= inv_eta; sum += A[i][k] * A[i][k]; }
        double sigma = sqrt(sum);
        if (A[k][k] < 0) sigma = -sigma;
        A[k][k] += sigma;
        A1[k] = sigma * A[k][k];
        A2[k] = -eta * sigma;
#pragma unroll
        for (int j = k + 1; j < 4; j++) {
            double s = 0;
#pragma unroll
            for (int i = k; i < 6; i++) s += A[i][k] * A[i][j];
            const double tau = s / A1[k];
#pragma unroll
            for (int i = k; i < 6; i++) A[i][j] -= tau * A[i][k];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double tau = 0;
#pragma unroll
        for (int i = j; i < 6; i++) tau += A[i][j] * b[i];
        tau /= A1[j];
#pragma unroll
        for (int i = j; i < 6; i++) b[i] -= tau * A[i][j];
    }
    x[3] = b[3] / A2[3];
#pragma unroll
    for (int i = 2; i >= 0; i--) {
        double s = 0;
#pragma unroll
        for (int j = i + 1; j < 4; j++) s += A[i][j] * x[j];
        x[i] = (b[i] - s) / A2[i];
    }
}
// gauss_newton :831-849 with compute_A_and_b_gauss_newton :803-829
PNP_FN void pnp_gauss_newton(const double L[6][10], const double rho[6], double be[4])
{
    for (int it = 0; it < 5; it++) {
        double A[6][4], b[6], x[4];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const double* l = L[i];
            A[i][0] = 2 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3];
            A[i][1] = l[1] * be[0] + 2 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3];
            A[i][2] = l[3] * be[0] + l[4] * be[1] + 2 * l[5] * be[2] + l[8] * be[3];
            A[i][3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2 * l[9] * be[3];
            b[i] = rho[i] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] + l[4] * be[1] * be[2] +
                             l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] + l[8] * be[2] * be[3] + l[9] * be[3] * be[3]);
        }
        pnp_qr_solve(A, b, x);
#pragma unroll
        for (int i = 0; i < 4; i++) be[i] += x[i];
    }
}
// betas[c] of candidate c = 0, 1, 2 (the reference's Betas[1..3])
PNP_FN void pnp_all_betas(const double basis[4][12], const double cws[4][3], double betas[3][4])
{
    double L[6][10], rho[6];
    pnp_L_rho(basis, cws, L, rho);
    pnp_betas_1(L, rho, betas[0]); pnp_gauss_newton(L, rho, betas[0]);
    pnp_betas_2(L, rho, betas[1]); pnp_gauss_newton(L, rho, betas[1]);
    pnp_betas_3(L, rho, betas[2]); pnp_gauss_newton(L, rho, betas[2]);
}

// ------------------------------------------------------------------------------------------ compute_R_and_t :642-653, in pieces
// compute_ccs :444-455
PNP_FN void pnp_ccs(const double betas[4], const double basis[4][12], double ccs[4][3])
{
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 4; i++) s += betas[i] * basis[i][3 * j + k];
            ccs[j][k] = s;
        }
}
// compute_pcs :457-466 for one point
PNP_FN void pnp_pc(const double a[4], const double ccs[4][3], double pc[3])
{
#pragma unroll
    for (int j = 0; j < 3; j++) pc[j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
}
// solve_for_sign :627-640, given the camera-frame z of the FIRST correspondence: negating the control points negates every pc exactly
PNP_FN void pnp_sign(double pc0z, double ccs[4][3])
{
    if (pc0z < 0.0)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 3; k++) ccs[j][k] = -ccs[j][k];
}
// estimate_R_and_t :599-617 from ABt = sum (pc - pc0)(pw - pw0)^T: R = U V^T of its SVD, the third row negated for det < 0, t = pc0 -
// R pw0.  A vanishing singular direction (a planar set) is completed to a right-handed U; the reference leaves its sign to OpenCV.
PNP_FN void pnp_R_t(const double abt[9], const double pc0[3], const double pw0[3], double Rt[12])
{
    double A[3][3], V[3][3], s[3], U[3][3];     // U[j] = left singular vector j
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) A[i][j] = abt[3 * i + j];
    pnp_onesided<3, 3>(A, V);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        s[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
#pragma unroll
        for (int k = 0; k < 3; k++) U[j][k] = A[k][j] / s[j];
    }
    const double smax = fmax(s[0], fmax(s[1], s[2])), tiny = 1e-14 * smax;
#define PNP_CROSS(d, a, b) { U[d][0] = U[a][1] * U[b][2] - U[a][2] * U[b][1]; U[d][1] = U[a][2] * U[b][0] - U[a][0] * U[b][2]; \
                             U[d][2] = U[a][0] * U[b][1] - U[a][1] * U[b][0]; }
    if (s[2] <= tiny && s[2] <= s[1] && s[2] <= s[0]) PNP_CROSS(2, 0, 1)
    else if (s[1] <= tiny && s[1] <= s[0]) PNP_CROSS(1, 2, 0)
    else if (s[0] <= tiny) PNP_CROSS(0, 1, 2)
#undef PNP_CROSS
    double R[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[i][j] = U[0][i] * V[j][0] + U[1][i] * V[j][1] + U[2][i] * V[j][2];
    const double det = R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
                       R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1];
    if (det < 0) { R[2][0] = -R[2][0]; R[2][1] = -R[2][1]; R[2][2] = -R[2][2]; }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Rt[3 * i + j] = R[i][j];
        Rt[9 + i] = pc0[i] - pnp_dot3(R[i], pw0);
    }
}
// one term of reprojection_error :541-558
PNP_FN double pnp_reproj(const double Rt[12], const double K[4], const double pw[3], const double uv[2])
{
    const double Xc = pnp_dot3(Rt, pw) + Rt[9], Yc = pnp_dot3(Rt + 3, pw) + Rt[10], inv_Zc = 1.0 / (pnp_dot3(Rt + 6, pw) + Rt[11]);
    const double ue = K[2] + K[0] * Xc * inv_Zc, ve = K[3] + K[1] * Yc * inv_Zc;
    return sqrt((uv[0] - ue) * (uv[0] - ue) + (uv[1] - ve) * (uv[1] - ve));
}

// ---------------------------------------------------------------------------------------------------- CheckInliers :299-330
// One correspondence, in the reference's types: Xc, Yc, invZc rounded to float from double expressions, ue / ve double, the
// distances and error2 float.  Compiled without floating-point contraction (the Makefile's -ffp-contract=off), so the flag is an exact
// function of the double pose.  max_err = mvMaxError[i] = sigma2 * th2 in float (:146).  A NaN error is an outlier.
PNP_FN bool pnp_inlier(const double Rt[12], const double K[4], float X, float Y, float Z, float u, float v, float max_err)
{
    const float Xc = (float)(Rt[0] * X + Rt[1] * Y + Rt[2] * Z + Rt[9]);
    const float Yc = (float)(Rt[3] * X + Rt[4] * Y + Rt[5] * Z + Rt[10]);
    const float invZc = (float)(1 / (Rt[6] * X + Rt[7] * Y + Rt[8] * Z + Rt[11]));
    const double ue = K[2] + K[0] * Xc * invZc;
    const double ve = K[3] + K[1] * Yc * invZc;
    const float distX = (float)(u - ue);
    const float distY = (float)(v - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_err;
}

// ------------------------------------------------------------------------------------------------------ compute_pose, serially
// P.get(i, pw, uv) returns correspondence i (add_correspondence :354-364: floats widened to double).  A and V are scratch for the
// 12x12 eigenproblem.  detail, when not null, receives PNP_DETAIL doubles.
template <class View, class Mat>
PNP_FN void pnp_compute_pose(const View& P, int n, const double K[4], Mat& A, Mat& V, double Rt[12], double* detail)
{
    double pw[3], uv[2], a[4];
    double c0[3] = { 0, 0, 0 }, cov[6] = { 0, 0, 0, 0, 0, 0 };
    for (int i = 0; i < n; i++) { P.get(i, pw, uv); c0[0] += pw[0]; c0[1] += pw[1]; c0[2] += pw[2]; }
    c0[0] /= n; c0[1] /= n; c0[2] /= n;
    for (int i = 0; i < n; i++) {
        P.get(i, pw, uv);
        const double d0 = pw[0] - c0[0], d1 = pw[1] - c0[1], d2 = pw[2] - c0[2];
        cov[0] += d0 * d0; cov[1] += d0 * d1; cov[2] += d0 * d2; cov[3] += d1 * d1; cov[4] += d1 * d2; cov[5] += d2 * d2;
    }
    double cws[4][3], ci[3][3];
    pnp_control_points(n, c0, cov, cws, ci);

    {
        double acc[78];                                   // the upper triangle of M^T M, summed in index order
#pragma unroll
        for (int e = 0; e < 78; e++) acc[e] = 0.0;
        for (int i = 0; i < n; i++) {
            double m1[12], m2[12];
            P.get(i, pw, uv);
            pnp_alphas(ci, c0, pw, a);
            pnp_rows_M(a, uv, K, m1, m2);
            int e = 0;
#pragma unroll
            for (int r = 0; r < 12; r++)
#pragma unroll
                for (int c = r; c < 12; c++) acc[e++] += m1[r] * m1[c] + m2[r] * m2[c];
        }
        int e = 0;
#pragma unroll
        for (int r = 0; r < 12; r++)
#pragma unroll
            for (int c = r; c < 12; c++) { A(r, c) = acc[e]; A(c, r) = acc[e]; e++; }
    }
    pnp_jacobi12(A, V);
    double basis[4][12], L[6][10], rho[6];
    pnp_basis(A, V, basis);
    pnp_L_rho(basis, cws, L, rho);

    // the three candidates in turn (:497-507) and the choice of N (:509-511) as they arrive: nothing here is indexed by the candidate
    double best_betas[4], e0 = 0.0, e1 = 0.0, e2 = 0.0, ebest = 0.0;
    int which = 0;
    for (int cand = 0; cand < 3; cand++) {
        double be[4], ccs[4][3], pc[3], pc0[3] = { 0, 0, 0 }, abt[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, Rc[12];
        if (cand == 0) pnp_betas_1(L, rho, be); else if (cand == 1) pnp_betas_2(L, rho, be); else pnp_betas_3(L, rho, be);
        pnp_gauss_newton(L, rho, be);
        pnp_ccs(be, basis, ccs);
        P.get(0, pw, uv); pnp_alphas(ci, c0, pw, a); pnp_pc(a, ccs, pc);
        pnp_sign(pc[2], ccs);
        for (int i = 0; i < n; i++) {
            P.get(i, pw, uv); pnp_alphas(ci, c0, pw, a); pnp_pc(a, ccs, pc);
            pc0[0] += pc[0]; pc0[1] += pc[1]; pc0[2] += pc[2];
        }
        pc0[0] /= n; pc0[1] /= n; pc0[2] /= n;
        for (int i = 0; i < n; i++) {
            P.get(i, pw, uv); pnp_alphas(ci, c0, pw, a); pnp_pc(a, ccs, pc);
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int k = 0; k < 3; k++) abt[3 * j + k] += (pc[j] - pc0[j]) * (pw[k] - c0[k]);
        }
        pnp_R_t(abt, pc0, c0, Rc);
        double sum2 = 0.0;
        for (int i = 0; i < n; i++) { P.get(i, pw, uv); sum2 += pnp_reproj(Rc, K, pw, uv); }
        const double e = sum2 / n;
        e0 = cand == 0 ? e : e0; e1 = cand == 1 ? e : e1; e2 = cand == 2 ? e : e2;
        if (cand == 0 || e < ebest) {
            which = cand; ebest = e;
#pragma unroll
            for (int k = 0; k < 12; k++) Rt[k] = Rc[k];
#pragma unroll
            for (int k = 0; k < 4; k++) best_betas[k] = be[k];
        }
    }
    if (detail) {
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 3; k++) detail[3 * j + k] = cws[j][k];
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int k = 0; k < 12; k++) detail[12 + 12 * r + k] = basis[r][k];
#pragma unroll
        for (int k = 0; k < 4; k++) detail[60 + k] = best_betas[k];
        detail[64] = e0; detail[65] = e1; detail[66] = e2; detail[67] = (double)(which + 1);
    }
}

// ----------------------------------------------------------------------------------------- the sampling loop :178-192
// idx[i] = vAvailableIndices[r[i]] with vAvailableIndices = 0 .. n-1 and position r[i] taking the last element after each draw.
// min_set <= 8 draws, so the list is the identity except at the positions written so far.
PNP_FN int pnp_avail(const int* pos, const int* val, int cnt, int p)
{
    int v = p;
    for (int j = 0; j < cnt; j++) if (pos[j] == p) v = val[j];       // the latest write to position p wins
    return v;
}
PNP_FN void pnp_sample(int n, int min_set, const int* r, int* idx)
{
    int pos[8], val[8];
    for (int i = 0; i < min_set; i++) {
        idx[i] = pnp_avail(pos, val, i, r[i]);
        pos[i] = r[i]; val[i] = pnp_avail(pos, val, i, n - 1 - i);   // vAvailableIndices[randi] = back(); pop_back()
    }
}
