// mpt_correct_kernels.hip -- device side of ccm_map_table_correct_frames (mpt_correct_host.cpp, include/ccm_hot.h "loop and merge
// corrections on the table"): the keyframe and map-point correction of LoopFinder::CorrectLoop (src/LoopFinder.cpp:543-613),
// MapMerger::MergeMaps (src/MapMerger.cpp:349-392), the tail of OptimizeEssentialGraph* (src/Optimizer.cpp:1279-1330) and the tail of
// the global BA (src/MapMerger.cpp:637-753) on keyframe handles and the map-point table.
//   k_mpt_correct_poses     thread per moved keyframe: its new Tcw / Ow into the call's staging block (cam_new)
//   k_mpt_correct           wave per listed point: the new position, then MapPoint::UpdateNormalAndDepth (src/MapPoint.cpp:779-823)
//                           with each observing keyframe's old or new camera centre, as the reference's loop order has it
//   k_mpt_correct_publish   cam_new into the handles' camera blocks
// k_mpt_correct reads the handles' OLD Tcw / Ow; the publish runs behind it on the same stream, so nothing is overwritten early.
// The Sim3 arithmetic is that of k_ess_correct_points (ess_kernels.hip) through the same functions of sim3_math.h, the normal and the
// depths that of k_mpt_refresh (mpt_kernels.hip), written a second time so that that kernel's code stays as it is.
// No atomics, no LDS, no scratch; every slot is checked against the capacity, every index has been checked by the host.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/ccm_hot.h"
#include "mpt_types.h"
#include "sim3_math.h"
#include "pose_camera.h"
#include "map_math.h"

// SIM3: [R | t / s] of CorrectedSiw (src/LoopFinder.cpp:604-611: eigt *= (1./s), toCvSE3) through ba_pose_to_camera, the definition
// the host copy uses.  RIGID: the caller's Tcw / Ow.
__global__ void k_mpt_correct_poses(MptCorrectArgs A)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n_moved) return;
    float* o = A.cam_new + (size_t)MPC_CAM_STRIDE * k;
    if (A.transform == CCM_MC_SIM3) {
        const double* S = A.sim3_after + 8 * (size_t)k;
        const double is = 1.0 / S[7];
        const double pose7[7] = { S[0], S[1], S[2], S[3], S[4] * is, S[5] * is, S[6] * is };
        float Tcw[12], Ow[3];
        ba_pose_to_camera(pose7, Tcw, Ow);
        for (int i = 0; i < 12; i++) o[i] = Tcw[i];
        for (int i = 0; i < 3; i++) o[12 + i] = Ow[i];
    } else {
        for (int i = 0; i < 12; i++) o[i] = A.Tcw_after[12 * (size_t)k + i];
        for (int i = 0; i < 3; i++) o[12 + i] = A.Ow_after[3 * (size_t)k + i];
    }
    o[15] = 0.0f;
}

// cv::norm of a float 3-vector: the squares summed in double (mpr_norm of mpt_kernels.hip)
__device__ inline double mpc_norm(float x, float y, float z)
{
    return sqrt(__dadd_rn(__dadd_rn(__dmul_rn((double)x, (double)x), __dmul_rn((double)y, (double)y)), __dmul_rn((double)z, (double)z)));
}
// The camera centre of keyframe j as point p's UpdateNormalAndDepth finds it.  POSES_FIRST: every moved keyframe has its new pose.
// IN_ORDER: keyframe j has it iff its SetPose came before the owner's points were refreshed, j < owner.
__device__ inline const float* mpc_Ow(const MptCorrectArgs& A, int j, int owner)
{
    const bool moved = j < A.n_moved && (A.order == CCM_MC_POSES_FIRST || j < owner);
    return moved ? A.cam_new + (size_t)MPC_CAM_STRIDE * j + 12 : A.kf[j].cam + 12;
}

// One wave per listed point, MPR_TPB / 64 points per workgroup (as k_mpt_refresh).  The transform is wave-uniform and done by every
// lane; the rays of the observations are computed 64 at a time and summed strictly in list order through __shfl.
__global__ __launch_bounds__(MPR_TPB) void k_mpt_correct(MptCorrectArgs A, MptTable T)
{
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, p = blockIdx.x * (MPR_TPB / 64) + wv;
    if (p >= A.n_points) return;
    const int s = A.slot[p];
    if (s < 0 || s >= T.capacity) return;                        // the host has checked it
    const int owner = A.owner[p];
    float P0 = T.pos[3 * (size_t)s], P1 = T.pos[3 * (size_t)s + 1], P2 = T.pos[3 * (size_t)s + 2];
    float n0 = T.normal[3 * (size_t)s], n1 = T.normal[3 * (size_t)s + 1], n2 = T.normal[3 * (size_t)s + 2];
    float mn = T.min_dist[s], mx = T.max_dist[s];
    if (owner >= 0 && owner < A.n_moved) {
        if (A.transform == CCM_MC_SIM3) {                        // correctedSwi.map(Siw.map(P)), as k_ess_correct_points
            double So[8], Sn[8], Si[8], P[3], Q[3], O[3];
            for (int k = 0; k < 8; k++) { So[k] = A.sim3_before[8LL * owner + k]; Sn[k] = A.sim3_after[8LL * owner + k]; }
            P[0] = (double)P0; P[1] = (double)P1; P[2] = (double)P2;         // Converter::toVector3d
            s3_rotv(So, P, Q);
            for (int k = 0; k < 3; k++) Q[k] = So[7] * Q[k] + So[4 + k];
            s3_inverse(Sn, Si);
            s3_rotv(Si, Q, O);
            P0 = (float)(Si[7] * O[0] + Si[4]); P1 = (float)(Si[7] * O[1] + Si[5]); P2 = (float)(Si[7] * O[2] + Si[6]);   // Converter::toCvMat
        } else {                                                 // Rwc * (Rcw_before * P + tcw_before) + twc
            const float* Tb = A.kf[owner].cam;
            const float* Ta = A.Tcw_after + 12 * (size_t)owner;
            const float* Oa = A.Ow_after + 3 * (size_t)owner;
            const float X[3] = { P0, P1, P2 };
            const float Xc[3] = { map_row(Tb, 0, X), map_row(Tb, 1, X), map_row(Tb, 2, X) };
            float Pn[3];
            for (int r = 0; r < 3; r++)
                Pn[r] = (float)(((double)Ta[r] * Xc[0] + (double)Ta[4 + r] * Xc[1] + (double)Ta[8 + r] * Xc[2]) + (double)Oa[r]);
            P0 = Pn[0]; P1 = Pn[1]; P2 = Pn[2];
        }
        if (lane == 0) { T.pos[3 * (size_t)s] = P0; T.pos[3 * (size_t)s + 1] = P1; T.pos[3 * (size_t)s + 2] = P2; }
        int c = 0, o0 = 0;
        if (A.obs_first) { o0 = A.obs_first[p]; c = A.obs_first[p + 1] - o0; }
        if (c > 0) {
            n0 = 0.0f; n1 = 0.0f; n2 = 0.0f;
            for (int base = 0; base < c; base += 64) {
                const int i = base + lane;
                float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
                if (i < c) {
                    const float* Ow = mpc_Ow(A, A.obs_kf[o0 + i], owner);
                    const float d0 = P0 - Ow[0], d1 = P1 - Ow[1], d2 = P2 - Ow[2];
                    const float a = (float)(1.0 / mpc_norm(d0, d1, d2));
                    v0 = __fmul_rn(d0, a); v1 = __fmul_rn(d1, a); v2 = __fmul_rn(d2, a);
                }
                const int m = min(64, c - base);
                for (int l = 0; l < m; l++) {                    // cv::scaleAdd, observation by observation
                    n0 = __fadd_rn(__shfl(v0, l, 64), n0); n1 = __fadd_rn(__shfl(v1, l, 64), n1); n2 = __fadd_rn(__shfl(v2, l, 64), n2);
                }
            }
            const float inv = (float)(1.0 / (double)c);          // Mat / n multiplies by the reciprocal
            n0 = __fmul_rn(n0, inv); n1 = __fmul_rn(n1, inv); n2 = __fmul_rn(n2, inv);
            const int rk = A.ref_kf[p];
            const MptCorrectKf& R = A.kf[rk];
            const float* Or = mpc_Ow(A, rk, owner);
            const float dist = (float)mpc_norm(P0 - Or[0], P1 - Or[1], P2 - Or[2]);
            const int level = min(max(R.oct[A.ref_feat[p]], 0), 255);   // within the handle's n_levels; sf holds 256 entries
            mx = __fmul_rn(dist, R.sf[level]);
            mn = __fdiv_rn(mx, R.sf[R.n_levels - 1]);
            if (lane == 0) {
                T.normal[3 * (size_t)s] = n0; T.normal[3 * (size_t)s + 1] = n1; T.normal[3 * (size_t)s + 2] = n2;
                T.min_dist[s] = mn; T.max_dist[s] = mx;
            }
        }
    }
    if (lane == 0) {                                             // the result block reports the row as it stands
        A.pos[3 * (size_t)p] = P0; A.pos[3 * (size_t)p + 1] = P1; A.pos[3 * (size_t)p + 2] = P2;
        A.normal[3 * (size_t)p] = n0; A.normal[3 * (size_t)p + 1] = n1; A.normal[3 * (size_t)p + 2] = n2;
        A.min_dist[p] = mn; A.max_dist[p] = mx;
    }
}

// 16 threads per moved keyframe, 15 of them write: Tcw [12] and Ow [3] of the handle's camera block
__global__ void k_mpt_correct_publish(MptCorrectArgs A)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, k = i / MPC_CAM_STRIDE, j = i % MPC_CAM_STRIDE;
    if (k >= A.n_moved || j >= 15) return;
    float* cam = A.kf[k].cam;
    if (cam) cam[j] = A.cam_new[(size_t)MPC_CAM_STRIDE * k + j];
}

void mpt_launch_correct(hipStream_t s, const MptCorrectArgs& A, const MptTable& T)
{
    if (A.n_moved > 0) hipLaunchKernelGGL(k_mpt_correct_poses, dim3((A.n_moved + 63) / 64), dim3(64), 0, s, A);
    if (A.n_points > 0) hipLaunchKernelGGL(k_mpt_correct, dim3((A.n_points + MPR_TPB / 64 - 1) / (MPR_TPB / 64)), dim3(MPR_TPB), 0, s, A, T);
    if (A.n_moved > 0) hipLaunchKernelGGL(k_mpt_correct_publish, dim3((A.n_moved * MPC_CAM_STRIDE + 255) / 256), dim3(256), 0, s, A);
}
