// frame_pose_host.cpp -- Optimizer::PoseOptimizationClient(Frame&) on a frame handle (src/Optimizer.cpp:215-347): the points come
// with the call (ccm_frame_pose_optimize) or from a map-point table (ccm_frame_pose_optimize_table).
// Staging: [ n_inliers+status | outlier | pose ] down, [ pose | intr | inv_sigma2 | (xyz) ] up; the pose sits at the seam.
#include "mpt_internal.h"

int frame_pose_queue(ccm_ctx* c, ccm_frame* f, int n_mp, const float* pos, const uint8_t* flags, int n_levels, const PoseIo& o)
{
    FrameState& S = *frame_state(c);
    hipStream_t st = c->stream;
    const int n = f->n;
    CCM_RESERVE(c, S.pts, (size_t)n * 24); CCM_RESERVE(c, S.obs, (size_t)n * 16); CCM_RESERVE(c, S.info, (size_t)n * 8);
    CCM_RESERVE(c, S.err, (size_t)n * 16); CCM_RESERVE(c, S.outl, (size_t)n); CCM_RESERVE(c, S.kof, (size_t)n * 4); CCM_RESERVE(c, S.first, 16);
    const Staging& G = S.stage;
    int* d_ninl = G.dev<int>(o.ninl); int* d_status = d_ninl + 1;
    PoseGatherArgs A{ n, f->kx, f->ky, f->oct, f->mp_id, n_mp, G.dev<double>(o.xyz), pos, flags, G.dev<float>(o.is2), n_levels,
                      S.first.as<int>(), S.pts.as<double>(), S.obs.as<double>(), S.info.as<double>(), S.kof.as<int>(), d_status };
    frame_launch_pose_gather(st, A);
    CCM_HIP(c, hipGetLastError());
    PoseDev D{ 1, G.dev<double>(o.pose), G.dev<double>(o.intr), S.first.as<int>(), S.pts.as<double>(), S.obs.as<double>(),
               S.info.as<double>(), S.err.as<double>(), S.outl.as<uint8_t>(), d_ninl };
    pose_launch(st, D);
    CCM_HIP(c, hipGetLastError());
    frame_launch_pose_scatter(st, n, S.kof.as<int>(), S.first.as<int>(), S.outl.as<uint8_t>(), G.dev<uint8_t>(o.outl));
    CCM_HIP(c, hipGetLastError());
    return CCM_OK;
}

int frame_pose_run(ccm_ctx* c, ccm_frame* f, int n_mp, const double* mp_xyz, const float* pos, const uint8_t* flags,
                   const float* inv_level_sigma2, int n_levels, const double intr[4], double pose7[7], uint8_t* outlier, int32_t* n_inliers,
                   bool* bad_id)
{
    CCM_HIP(c, hipSetDevice(c->device));
    Staging& G = frame_state(c)->stage;
    const int n = f->n;
    const size_t xyz_bytes = mp_xyz ? (size_t)n_mp * 24 : 0;
    size_t off = 0;
    const size_t o_ninl = seg(off, 16), o_outl = seg(off, (size_t)n), o_pose = seg(off, 56);
    const size_t res_end = o_pose + 56;
    const size_t o_intr = seg(off, 32), o_is2 = seg(off, (size_t)n_levels * 4), o_xyz = seg(off, xyz_bytes);
    const size_t end = off;
    int rc;
    if ((rc = G.reserve(c, end))) return rc;
    G.put(o_pose, pose7, 56); G.put(o_intr, intr, 32);
    G.put(o_is2, inv_level_sigma2, (size_t)n_levels * 4);
    G.put(o_xyz, mp_xyz, xyz_bytes);
    if ((rc = G.upload(c, o_pose, end))) return rc;
    if ((rc = frame_pose_queue(c, f, n_mp, pos, flags, n_levels, PoseIo{ o_ninl, o_outl, o_pose, o_intr, o_is2, o_xyz }))) return rc;
    if ((rc = G.download(c, 0, res_end)) || (rc = G.wait(c))) return rc;
    int head[2];
    G.get(head, o_ninl, 8);
    *bad_id = head[1] != 0;
    if (*bad_id) return CCM_OK;
    G.get(pose7, o_pose, 56);
    G.get(outlier, o_outl, n);
    *n_inliers = head[0];
    return CCM_OK;
}

extern "C" {

// Optimizer::PoseOptimizationClient(Frame&), src/Optimizer.cpp:215-347, the frame's correspondences gathered on the device
int ccm_frame_pose_optimize(ccm_ctx* c, ccm_frame* f, int n_mp, const double* mp_xyz, const float* inv_level_sigma2, int n_levels,
                            const double intr[4], double pose7[7], uint8_t* outlier, int32_t* n_inliers)
{
    RoctxRange roctx_("ccm_frame_pose_optimize");
    if (!c || !f) return CCM_E_ARG;
    int rc = frame_check(c, f);
    if (rc) return rc;
    if (!intr || !pose7 || !n_inliers || n_mp < 0 || (n_mp > 0 && !mp_xyz) || (f->n > 0 && (!outlier || !inv_level_sigma2 || n_levels < 1)))
        return ccm_fail(c, CCM_E_ARG, "bad pose arguments");
    if (f->n == 0) { *n_inliers = 0; return CCM_OK; }
    return ccm_guard(c, "ccm_frame_pose_optimize", [&]() -> int {
        bool bad_id = false;
        if ((rc = frame_pose_run(c, f, n_mp, mp_xyz, nullptr, nullptr, inv_level_sigma2, n_levels, intr, pose7, outlier, n_inliers, &bad_id))) return rc;
        if (bad_id) return ccm_fail(c, CCM_E_ARG, "a map-point id outside [0, %d) or an octave outside [0, %d)", n_mp, n_levels);
        return CCM_OK;
    });
}

// Optimizer::PoseOptimizationClient(Frame&), src/Optimizer.cpp:215-347, the points read from the table
int ccm_frame_pose_optimize_table(ccm_ctx* c, ccm_frame* f, ccm_map_table* t, const float* inv_level_sigma2, int n_levels,
                                  const double intr[4], double pose7[7], uint8_t* outlier, int32_t* n_inliers)
{
    RoctxRange roctx_("ccm_frame_pose_optimize_table");
    if (!c || !f || !t) return CCM_E_ARG;
    int rc = frame_check(c, f);
    if (rc || (rc = check_table(c, t))) return rc;
    if (!intr || !pose7 || !n_inliers || (f->n > 0 && (!outlier || !inv_level_sigma2 || n_levels < 1)))
        return ccm_fail(c, CCM_E_ARG, "bad pose arguments");
    if (f->n == 0) { *n_inliers = 0; return CCM_OK; }
    return table_call(c, t, false, "ccm_frame_pose_optimize_table", [&]() -> int {
        bool bad_id = false;
        if ((rc = frame_pose_run(c, f, t->T.capacity, nullptr, t->T.pos, t->T.flags, inv_level_sigma2, n_levels, intr, pose7, outlier, n_inliers, &bad_id)))
            return rc;
        if (bad_id) return ccm_fail(c, CCM_E_ARG, "a map-point id outside the table or of a slot that is not LIVE, or an octave outside [0, %d)", n_levels);
        return CCM_OK;
    });
}

}  // extern "C"
