// ba_table_host.cpp -- ccm_ba_solve_table_frames (include/ccm_hot.h "local BA on the table"): Optimizer::LocalBundleAdjustmentClient
// (src/Optimizer.cpp:349-644) on keyframe handles and the map-point table.  This file holds the checks, the staging layout, the lock on
// the table's rows and the handles' host copies; the solve is ccm_ba_solve's (ba_host.cpp), with the two kernels of ba_table.hip in
// place of the uploads of observations, information values and points and of the download of the points.
#include "mpt_internal.h"
#include "ba_table.h"
#include "ba_launch.h"
#include "pose_camera.h"
#include "map_math.h"
#include <cstddef>
#include <unordered_set>

static_assert(offsetof(MapCam, Ow) == offsetof(MapCam, Tcw) + 48, "BaTableKf::cam: Tcw [12] then Ow [3]");

extern "C" {

int ccm_pose_to_camera(const double* pose7, float* Tcw12, float* Ow3)
{
    if (!pose7 || !Tcw12 || !Ow3) return CCM_E_ARG;
    ba_pose_to_camera(pose7, Tcw12, Ow3);
    return CCM_OK;
}

int ccm_ba_solve_table_frames(ccm_ctx* c, ccm_map_table* t, ccm_ba_table_problem* tp, const ccm_ba_options* opt, ccm_ba_result* res)
{
    if (!c || !t || !tp || !opt) return CCM_E_ARG;
    const char* fn = "ccm_ba_solve_table_frames";
    int rc = check_table(c, t);
    if (rc) return rc;
    if (comm_ranks(c) > 1) return ccm_fail(c, CCM_E_STATE, "%s: the context has a communicator of %d ranks; the table route is unsharded", fn, comm_ranks(c));
    if (tp->n_kf <= 0 || tp->n_points < 0) return ccm_fail(c, CCM_E_ARG, "%s: n_kf = %d, n_points = %d", fn, tp->n_kf, tp->n_points);
    if (!tp->kfs || !tp->poses || !tp->fixed || !tp->intr || !tp->inv_level_sigma2)
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !tp->kfs ? "kfs" : !tp->poses ? "poses" : !tp->fixed ? "fixed" : !tp->intr ? "intr" : "inv_level_sigma2");
    if (tp->n_points > 0 && (!tp->slot || !tp->obs_first)) return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !tp->slot ? "slot" : "obs_first");
    if (tp->n_levels < 1 || tp->n_levels > CCM_MAX_LEVELS) return ccm_fail(c, CCM_E_ARG, "%s: n_levels = %d outside [1, %d]", fn, tp->n_levels, CCM_MAX_LEVELS);
    bool synced = false;
    return table_call(c, t, true, fn, [&]() -> int {
        const int P = tp->n_kf, L = tp->n_points;
        // ---- checks: nothing is queued and nothing written before the last of them
        if (L > 0 && tp->obs_first[0] != 0) return ccm_fail(c, CCM_E_ARG, "%s: obs_first[0] = %d, not 0", fn, tp->obs_first[0]);
        for (int p = 0; p < L; p++)
            if (tp->obs_first[p + 1] < tp->obs_first[p])
                return ccm_fail(c, CCM_E_ARG, "%s: obs_first[%d] = %d below obs_first[%d] = %d", fn, p + 1, tp->obs_first[p + 1], p, tp->obs_first[p]);
        const int E = L > 0 ? tp->obs_first[L] : 0;
        if (E > 0 && (!tp->obs_kf || !tp->obs_feat)) return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !tp->obs_kf ? "obs_kf" : "obs_feat");
        {
            std::unordered_set<const ccm_frame*> seen_kf;
            for (int k = 0; k < P; k++) {
                const ccm_frame* f = tp->kfs[k];
                if ((rc = frame_named_check(c, f, CCM_E_STATE, fn, "kfs[%d]", k))) return rc;
                if (!seen_kf.insert(f).second) return ccm_fail(c, CCM_E_ARG, "%s: kfs[%d] is listed twice", fn, k);
                if (tp->n_levels < f->n_levels) return ccm_fail(c, CCM_E_ARG, "%s: n_levels = %d below the %d of kfs[%d]", fn, tp->n_levels, f->n_levels, k);
            }
        }
        for (int p = 0; p < L; p++)
            for (int e = tp->obs_first[p]; e < tp->obs_first[p + 1]; e++) {
                const int k = tp->obs_kf[e];
                if (k < 0 || k >= P) return ccm_fail(c, CCM_E_ARG, "%s: point %d, entry %d: keyframe %d outside [0, %d)", fn, p, e, k, P);
                if (tp->obs_feat[e] < 0 || tp->obs_feat[e] >= tp->kfs[k]->n)
                    return ccm_fail(c, CCM_E_ARG, "%s: point %d, entry %d: feature %d outside [0, %d) of kfs[%d]", fn, p, e, tp->obs_feat[e], tp->kfs[k]->n, k);
            }
        bool dup = false;
        if ((rc = mark_slots(c, t, L, tp->slot, &dup))) return rc;
        if (dup) return ccm_fail(c, CCM_E_ARG, "%s: a slot is listed twice", fn);

        CCM_HIP(c, hipSetDevice(c->device));
        // ---- the array problem's vertices and edge ends; observations, information values and points stay where they are
        std::vector<int32_t> edge_point((size_t)E);
        for (int p = 0; p < L; p++) for (int e = tp->obs_first[p]; e < tp->obs_first[p + 1]; e++) edge_point[e] = p;
        ccm_ba_problem pb{};
        pb.n_poses = P; pb.poses = tp->poses; pb.fixed = tp->fixed; pb.intr = tp->intr;
        pb.n_points = L; pb.n_edges = E; pb.edge_pose = tp->obs_kf; pb.edge_point = edge_point.data();

        // ---- staging (ba_table.h)
        const size_t mp = (size_t)P, ml = (size_t)L, me = (size_t)E;
        BaTableRoute R;
        size_t off = 0;
        R.o_pose_out = seg(off, mp * 56); R.o_outl = seg(off, me); R.o_pos = seg(off, ml * 12);
        R.res_end = R.in_begin = off;
        R.o_pose_in = seg(off, mp * 56); R.o_intr = seg(off, mp * 32);
        const size_t o_slot = seg(off, ml * 4);
        R.o_feat = seg(off, me * 4);
        const size_t o_view = seg(off, mp * sizeof(BaTableKf)), o_lev = seg(off, (size_t)tp->n_levels * 4), o_pub = seg(off, mp);
        R.in_end = off;
        Staging& G = frame_state(c)->stage;
        if ((rc = G.reserve(c, off))) return rc;
        // (the staging area is there: from here on only the device can fail)
        // a published handle without a keyframe block gets one, as ccm_frame_set_pose would give it (its camera is all zero until then)
        for (int k = 0; k < P; k++) {
            ccm_frame* f = tp->kfs[k];
            if (!tp->publish || !tp->publish[k] || f->kf_mem) continue;
            if ((rc = kf_block(c, f))) return rc;
            CCM_HIP(c, hipMemsetAsync(f->d_cam, 0, sizeof(MapCam), c->stream));
        }
        G.put(R.o_pose_in, tp->poses, mp * 56); G.put(R.o_intr, tp->intr, mp * 32);
        G.put(o_slot, tp->slot, ml * 4); G.put(o_lev, tp->inv_level_sigma2, (size_t)tp->n_levels * 4);
        uint8_t* pub = G.host<uint8_t>(o_pub);
        BaTableKf* hv = G.host<BaTableKf>(o_view);
        for (int k = 0; k < P; k++) {
            const ccm_frame* f = tp->kfs[k];
            pub[k] = tp->publish && tp->publish[k] ? 1 : 0;
            hv[k] = BaTableKf{ f->kx, f->ky, f->oct, pub[k] ? (float*)((uint8_t*)f->d_cam + offsetof(MapCam, Tcw)) : nullptr };
        }
        R.G = &G; R.obs_feat = tp->obs_feat; R.pos_out = tp->pos_out;
        R.A.n_levels = tp->n_levels; R.A.kf = G.dev<BaTableKf>(o_view); R.A.slot = G.dev<int>(o_slot);
        R.A.level_info = G.dev<float>(o_lev); R.A.publish = G.dev<uint8_t>(o_pub);
        R.A.table_pos = t->T.pos; R.A.pos_out = G.dev<float>(R.o_pos);

        if ((rc = ba_solve_table(c, &pb, opt, res, &R))) return rc;
        synced = true;                                                       // the solve ends in the staging block's wait
        // ---- the handles' host copies, brought to the bits the device wrote
        if (R.wrote)
            for (int k = 0; k < P; k++) {
                if (!pub[k]) continue;
                ccm_frame* f = tp->kfs[k];
                ba_pose_to_camera(tp->poses + 7 * (size_t)k, f->cam.Tcw, f->cam.Ow);
                f->has_pose = true;
            }
        return CCM_OK;
    }, &synced);
}

}  // extern "C"
