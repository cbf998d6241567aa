// sim3_host.cpp -- C ABI of the batched Optimizer::OptimizeSim3 (cslam/src/Optimizer.cpp:867-1062); the whole
// schedule of every problem runs in one kernel launch (sim3_kernels.hip).
#include "sim3_internal.h"
#include <algorithm>

void sim3_state_free(Sim3State* s) { delete s; }

extern "C" int ccm_optimize_sim3(ccm_ctx* c, ccm_sim3_problem* pb)
{
    RoctxRange roctx_("ccm_optimize_sim3");
    return ccm_guard(c, "ccm_optimize_sim3", [&]() -> int {
        if (!c || !pb) return CCM_E_ARG;
        if (pb->n_problems == 0) return CCM_OK;
        if (pb->n_problems < 0 || !pb->sim3 || !pb->fix_scale || !pb->K1 || !pb->K2 || !pb->first || !pb->th2 || !pb->n_inliers)
            return ccm_fail(c, CCM_E_ARG, "bad Sim3 problem");
        const int F = pb->n_problems;
        if (pb->first[0] != 0) return ccm_fail(c, CCM_E_ARG, "first[0] must be 0");
        for (int f = 0; f < F; f++) if (pb->first[f + 1] < pb->first[f]) return ccm_fail(c, CCM_E_ARG, "first[] must be non-decreasing");
        const size_t T = (size_t)pb->first[F];
        if (T > 0 && (!pb->P1 || !pb->P2 || !pb->obs1 || !pb->obs2 || !pb->info1 || !pb->info2 || !pb->inlier))
            return ccm_fail(c, CCM_E_ARG, "bad Sim3 problem");
        CCM_HIP(c, hipSetDevice(c->device));
        if (!c->sim3) c->sim3 = new Sim3State();
        Sim3State& S = *c->sim3;
        hipStream_t st = c->stream;
        int rc;
        if ((rc = ccm_upload(c, S.sim3, pb->sim3, (size_t)F * 64, st))) return rc;
        if ((rc = ccm_upload(c, S.fix, pb->fix_scale, (size_t)F * 4, st))) return rc;
        if ((rc = ccm_upload(c, S.K1, pb->K1, (size_t)F * 32, st))) return rc;
        if ((rc = ccm_upload(c, S.K2, pb->K2, (size_t)F * 32, st))) return rc;
        if ((rc = ccm_upload(c, S.first, pb->first, ((size_t)F + 1) * 4, st))) return rc;
        if ((rc = ccm_upload(c, S.th2, pb->th2, (size_t)F * 4, st))) return rc;
        if ((rc = ccm_upload(c, S.P1, pb->P1, T * 24, st))) return rc;
        if ((rc = ccm_upload(c, S.P2, pb->P2, T * 24, st))) return rc;
        if ((rc = ccm_upload(c, S.o1, pb->obs1, T * 16, st))) return rc;
        if ((rc = ccm_upload(c, S.o2, pb->obs2, T * 16, st))) return rc;
        if ((rc = ccm_upload(c, S.i1, pb->info1, T * 8, st))) return rc;
        if ((rc = ccm_upload(c, S.i2, pb->info2, T * 8, st))) return rc;
        CCM_RESERVE(c, S.err, std::max<size_t>(T * 32, 16)); CCM_RESERVE(c, S.inl, std::max<size_t>(T, 16));
        CCM_RESERVE(c, S.nin, (size_t)F * 4);
        Sim3Dev D{ F, S.sim3.as<double>(), S.fix.as<int>(), S.K1.as<double>(), S.K2.as<double>(), S.first.as<int>(), S.P1.as<double>(),
                   S.P2.as<double>(), S.o1.as<double>(), S.o2.as<double>(), S.i1.as<double>(), S.i2.as<double>(), S.th2.as<float>(),
                   S.err.as<double>(), S.inl.as<uint8_t>(), S.nin.as<int>() };
        sim3_launch(st, D);
        CCM_HIP(c, hipGetLastError());
        CCM_HIP(c, hipMemcpyAsync(pb->sim3, S.sim3.p, (size_t)F * 64, hipMemcpyDeviceToHost, st));
        if (T) CCM_HIP(c, hipMemcpyAsync(pb->inlier, S.inl.p, T, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipMemcpyAsync(pb->n_inliers, S.nin.p, (size_t)F * 4, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipStreamSynchronize(st));
        return CCM_OK;
    });
}
