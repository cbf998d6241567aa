// pose_host.cpp -- C ABI of the batched pose-only optimisation (Optimizer::PoseOptimizationClient,
// src/Optimizer.cpp:215-347); the whole schedule runs in one kernel launch (pose_kernels.hip).
#include "ccm_internal.h"
#include "pose_types.h"
#include <algorithm>

struct PoseState { DevBuf poses, intr, first, pts, obs, info, err, outlier, ninl; };
static PoseState* pose_state(ccm_ctx* c)
{
    // lives with the BA state's lifetime rules: allocated on first use, freed with the context
    static_assert(sizeof(void*) == 8, "64-bit only");
    if (!c->pose) c->pose = new PoseState();
    return c->pose;
}
void pose_state_free(PoseState* s) { delete s; }

extern "C" int ccm_pose_optimize(ccm_ctx* c, ccm_pose_problem* pb)
{
    RoctxRange roctx_("ccm_pose_optimize");
    return ccm_guard(c, "ccm_pose_optimize", [&]() -> int {
        if (!c || !pb) return CCM_E_ARG;
        if (pb->n_frames == 0) return CCM_OK;
        if (pb->n_frames < 0 || !pb->poses || !pb->intr || !pb->first || !pb->n_inliers) return ccm_fail(c, CCM_E_ARG, "bad pose problem");
        const int F = pb->n_frames;
        if (pb->first[0] != 0) return ccm_fail(c, CCM_E_ARG, "first[0] must be 0");
        for (int f = 0; f < F; f++) if (pb->first[f + 1] < pb->first[f]) return ccm_fail(c, CCM_E_ARG, "first[] must be non-decreasing");
        const size_t T = (size_t)pb->first[F];
        if (T > 0 && (!pb->points || !pb->obs || !pb->info || !pb->outlier)) return ccm_fail(c, CCM_E_ARG, "bad pose problem");
        CCM_HIP(c, hipSetDevice(c->device));
        PoseState& S = *pose_state(c);
        hipStream_t st = c->stream;
        int rc;
        if ((rc = ccm_upload(c, S.poses, pb->poses, (size_t)F * 56, st))) return rc;
        if ((rc = ccm_upload(c, S.intr, pb->intr, (size_t)F * 32, st))) return rc;
        if ((rc = ccm_upload(c, S.first, pb->first, ((size_t)F + 1) * 4, st))) return rc;
        if ((rc = ccm_upload(c, S.pts, pb->points, T * 24, st))) return rc;
        if ((rc = ccm_upload(c, S.obs, pb->obs, T * 16, st))) return rc;
        if ((rc = ccm_upload(c, S.info, pb->info, T * 8, st))) return rc;
        CCM_RESERVE(c, S.err, std::max<size_t>(T * 16, 16)); CCM_RESERVE(c, S.outlier, std::max<size_t>(T, 16));
        CCM_RESERVE(c, S.ninl, (size_t)F * 4);
        PoseDev D{ F, S.poses.as<double>(), S.intr.as<double>(), S.first.as<int>(), S.pts.as<double>(), S.obs.as<double>(),
                   S.info.as<double>(), S.err.as<double>(), S.outlier.as<uint8_t>(), S.ninl.as<int>() };
        pose_launch(st, D);
        CCM_HIP(c, hipGetLastError());
        CCM_HIP(c, hipMemcpyAsync(pb->poses, S.poses.p, (size_t)F * 56, hipMemcpyDeviceToHost, st));
        if (T) CCM_HIP(c, hipMemcpyAsync(pb->outlier, S.outlier.p, T, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipMemcpyAsync(pb->n_inliers, S.ninl.p, (size_t)F * 4, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipStreamSynchronize(st));
        return CCM_OK;
    });
}
