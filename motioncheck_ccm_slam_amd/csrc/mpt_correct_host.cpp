// mpt_correct_host.cpp -- ccm_map_table_correct_frames (include/ccm_hot.h "loop and merge corrections on the table"): the keyframe
// and map-point correction of LoopFinder::CorrectLoop (src/LoopFinder.cpp:543-613), MapMerger::MergeMaps (src/MapMerger.cpp:349-392),
// the tail of OptimizeEssentialGraph* (src/Optimizer.cpp:1279-1330) and the tail of the global BA (src/MapMerger.cpp:637-753) on
// keyframe handles and the map-point table.  This file holds the checks, the staging layout, the lock on the table's rows and the
// handles' host copies; the arithmetic is in mpt_correct_kernels.hip.
// Staging: [ pos | normal | min_dist | max_dist ] down, [ slot | owner | obs_first | obs_kf | obs_feat | ref_kf | ref_feat | the Sim3
// pairs or the poses | views ] up, and behind them cam_new, which only the device writes.
#include "mpt_internal.h"
#include "pose_camera.h"
#include "map_math.h"
#include <cmath>
#include <cstddef>
#include <unordered_set>

static_assert(offsetof(MapCam, Ow) == offsetof(MapCam, Tcw) + 48, "MptCorrectKf::cam: Tcw [12] then Ow [3]");

// SIM3: the pose7 of [R | t / s] (src/LoopFinder.cpp:604-611: eigt *= (1./s)), as k_mpt_correct_poses forms it
static inline void correct_pose7(const double* S, double* pose7)
{
    const double is = 1.0 / S[7];
    for (int i = 0; i < 4; i++) pose7[i] = S[i];
    for (int i = 0; i < 3; i++) pose7[4 + i] = S[4 + i] * is;
}

extern "C" int ccm_map_table_correct_frames(ccm_ctx* c, ccm_map_table* t, const ccm_map_correct* u)
{
    RoctxRange roctx_("ccm_map_table_correct_frames");
    if (!c || !t || !u) return CCM_E_ARG;
    const char* fn = "ccm_map_table_correct_frames";
    int rc = check_table(c, t);
    if (rc) return rc;
    if (u->transform != CCM_MC_SIM3 && u->transform != CCM_MC_RIGID) return ccm_fail(c, CCM_E_ARG, "%s: transform = %d", fn, u->transform);
    if (u->order != CCM_MC_POSES_FIRST && u->order != CCM_MC_IN_ORDER) return ccm_fail(c, CCM_E_ARG, "%s: order = %d", fn, u->order);
    const bool sim3 = u->transform == CCM_MC_SIM3;
    if (u->n_kf < 0 || (u->n_kf > 0 && !u->kfs)) return ccm_fail(c, CCM_E_ARG, "%s: n_kf = %d%s", fn, u->n_kf, u->n_kf > 0 ? " and null kfs" : "");
    if (u->n_moved < 0 || u->n_moved > u->n_kf) return ccm_fail(c, CCM_E_ARG, "%s: n_moved = %d outside [0, %d]", fn, u->n_moved, u->n_kf);
    if (u->n_points < 0) return ccm_fail(c, CCM_E_ARG, "%s: n_points = %d", fn, u->n_points);
    if (u->n_moved > 0 && (sim3 ? !u->sim3_before || !u->sim3_after : !u->Tcw_after || !u->Ow_after))
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, sim3 ? (!u->sim3_before ? "sim3_before" : "sim3_after") : (!u->Tcw_after ? "Tcw_after" : "Ow_after"));
    const bool lists = u->obs_first != nullptr;
    if (u->n_points > 0 && (!u->slot || !u->owner || (lists && (!u->ref_kf || !u->ref_feat))))
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !u->slot ? "slot" : !u->owner ? "owner" : !u->ref_kf ? "ref_kf" : "ref_feat");
    if (u->n_moved == 0 && u->n_points == 0) return CCM_OK;
    bool synced = false;                                                       // writes rows; with an output it waits for them
    return table_call(c, t, true, fn, [&]() -> int {
        const int n = u->n_points, n_kf = u->n_kf, n_moved = u->n_moved;
        // ---- checks: nothing is queued and nothing written before the last of them
        int n_obs = 0;
        if (lists && n > 0) {
            if (u->obs_first[0] != 0) return ccm_fail(c, CCM_E_ARG, "%s: obs_first[0] = %d, not 0", fn, u->obs_first[0]);
            for (int p = 0; p < n; p++)
                if (u->obs_first[p + 1] < u->obs_first[p])
                    return ccm_fail(c, CCM_E_ARG, "%s: obs_first[%d] = %d below obs_first[%d] = %d", fn, p + 1, u->obs_first[p + 1], p, u->obs_first[p]);
            n_obs = u->obs_first[n];
            if (n_obs > 0 && (!u->obs_kf || !u->obs_feat)) return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !u->obs_kf ? "obs_kf" : "obs_feat");
        }
        {
            std::unordered_set<const ccm_frame*> seen_kf;
            for (int k = 0; k < n_kf; k++) {
                const ccm_frame* f = u->kfs[k];
                if ((rc = frame_named_check(c, f, CCM_E_STATE, fn, "kfs[%d]", k))) return rc;
                if (!seen_kf.insert(f).second) return ccm_fail(c, CCM_E_ARG, "%s: kfs[%d] is listed twice", fn, k);
            }
        }
        if (sim3)
            for (int k = 0; k < n_moved; k++) {
                for (int i = 0; i < 8; i++)
                    if (!std::isfinite(u->sim3_before[8 * (size_t)k + i]) || !std::isfinite(u->sim3_after[8 * (size_t)k + i]))
                        return ccm_fail(c, CCM_E_ARG, "%s: keyframe %d: entry %d of %s is not finite", fn, k, i,
                                        !std::isfinite(u->sim3_before[8 * (size_t)k + i]) ? "sim3_before" : "sim3_after");
                if (!(u->sim3_after[8 * (size_t)k + 7] > 0.0)) return ccm_fail(c, CCM_E_ARG, "%s: keyframe %d: scale %g of sim3_after", fn, k, u->sim3_after[8 * (size_t)k + 7]);
            }
        std::vector<uint8_t> used((size_t)n_kf, 0);   // 1: observed, 2: a reference keyframe, 4: owner of a point (points that move only)
        for (int p = 0; p < n; p++) {
            const int o = u->owner[p];
            if (o < -1 || o >= n_moved) return ccm_fail(c, CCM_E_ARG, "%s: point %d: owner %d outside [-1, %d)", fn, p, o, n_moved);
            if (o >= 0) used[o] |= 4;
            if (!lists) continue;
            for (int e = u->obs_first[p]; e < u->obs_first[p + 1]; e++) {
                const int k = u->obs_kf[e];
                if (k < 0 || k >= n_kf) return ccm_fail(c, CCM_E_ARG, "%s: point %d, entry %d: keyframe %d outside [0, %d)", fn, p, e, k, n_kf);
                if (u->obs_feat[e] < 0 || u->obs_feat[e] >= u->kfs[k]->n)
                    return ccm_fail(c, CCM_E_ARG, "%s: point %d, entry %d: feature %d outside [0, %d) of kfs[%d]", fn, p, e, u->obs_feat[e], u->kfs[k]->n, k);
                if (o >= 0) used[k] |= 1;
            }
            if (u->obs_first[p + 1] > u->obs_first[p]) {
                const int k = u->ref_kf[p];
                if (k < 0 || k >= n_kf) return ccm_fail(c, CCM_E_ARG, "%s: point %d: reference keyframe %d outside [0, %d)", fn, p, k, n_kf);
                if (u->ref_feat[p] < 0 || u->ref_feat[p] >= u->kfs[k]->n)
                    return ccm_fail(c, CCM_E_ARG, "%s: point %d: reference feature %d outside [0, %d) of kfs[%d]", fn, p, u->ref_feat[p], u->kfs[k]->n, k);
                if (o >= 0) used[k] |= 2;
            }
        }
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* f = u->kfs[k];
            if (!sim3 && (used[k] & 4) && !f->has_pose) return ccm_fail(c, CCM_E_STATE, "%s: kfs[%d] owns a point and has no pose", fn, k);
            if ((used[k] & 1) && !f->has_pose) return ccm_fail(c, CCM_E_STATE, "%s: kfs[%d] is observed and has no pose", fn, k);
            if ((used[k] & 2) && (!f->has_pose || !f->has_cam))
                return ccm_fail(c, CCM_E_STATE, "%s: kfs[%d] is a reference keyframe and has no %s", fn, k, !f->has_pose ? "pose" : "camera");
        }
        bool dup = false;
        if ((rc = mark_slots(c, t, n, u->slot, &dup))) return rc;
        if (dup) return ccm_fail(c, CCM_E_ARG, "%s: a slot is listed twice", fn);

        CCM_HIP(c, hipSetDevice(c->device));
        const size_t m = (size_t)n, mo = (size_t)n_obs, mk = (size_t)n_moved;
        size_t off = 0;
        const size_t o_pos = seg(off, m * 12), o_nrm = seg(off, m * 12), o_min = seg(off, m * 4), o_max = seg(off, m * 4);
        const size_t res_end = off;
        const size_t o_slot = seg(off, m * 4), o_owner = seg(off, m * 4);
        const size_t o_first = seg(off, lists ? (m + 1) * 4 : 0), o_okf = seg(off, mo * 4), o_ofeat = seg(off, mo * 4);
        const size_t o_rkf = seg(off, lists ? m * 4 : 0), o_rfeat = seg(off, lists ? m * 4 : 0);
        const size_t o_a = seg(off, sim3 ? mk * 64 : mk * 48), o_b = seg(off, sim3 ? mk * 64 : mk * 12);   // before | after, or Tcw | Ow
        const size_t o_view = seg(off, (size_t)n_kf * sizeof(MptCorrectKf));
        const size_t end = off;
        const size_t o_cam = seg(off, mk * MPC_CAM_STRIDE * 4);
        Staging& G = frame_state(c)->stage;
        if ((rc = G.reserve(c, off))) return rc;
        // (the staging area is there: from here on only the device can fail)
        // a moved handle without a keyframe block gets one, as ccm_frame_set_pose would give it (its camera is all zero until then)
        for (int k = 0; k < n_moved; k++) {
            ccm_frame* f = u->kfs[k];
            if (f->kf_mem) continue;
            if ((rc = kf_block(c, f))) return rc;
            CCM_HIP(c, hipMemsetAsync(f->d_cam, 0, sizeof(MapCam), c->stream));
        }
        G.put(o_slot, u->slot, m * 4); G.put(o_owner, u->owner, m * 4);
        if (lists && n > 0) {
            G.put(o_first, u->obs_first, (m + 1) * 4); G.put(o_okf, u->obs_kf, mo * 4); G.put(o_ofeat, u->obs_feat, mo * 4);
            int32_t* rk = G.host<int32_t>(o_rkf); int32_t* rf = G.host<int32_t>(o_rfeat);
            for (int p = 0; p < n; p++) {                        // not read for a point without observations: any value the caller left
                const bool has = u->obs_first[p + 1] > u->obs_first[p];
                rk[p] = has ? u->ref_kf[p] : 0; rf[p] = has ? u->ref_feat[p] : 0;
            }
        }
        if (sim3) { G.put(o_a, u->sim3_before, mk * 64); G.put(o_b, u->sim3_after, mk * 64); }
        else { G.put(o_a, u->Tcw_after, mk * 48); G.put(o_b, u->Ow_after, mk * 12); }
        MptCorrectKf* hv = G.host<MptCorrectKf>(o_view);
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* f = u->kfs[k];
            hv[k] = MptCorrectKf{ f->d_cam ? (float*)((uint8_t*)f->d_cam + offsetof(MapCam, Tcw)) : nullptr, f->oct, f->sf, f->cam_levels, 0 };
        }
        if ((rc = G.upload(c, o_slot, end))) return rc;
        MptCorrectArgs A{};
        A.n_points = n; A.n_moved = n_moved; A.transform = u->transform; A.order = u->order;
        A.slot = G.dev<int>(o_slot); A.owner = G.dev<int>(o_owner);
        if (lists && n > 0) {
            A.obs_first = G.dev<int>(o_first); A.obs_kf = G.dev<int>(o_okf); A.obs_feat = G.dev<int>(o_ofeat);
            A.ref_kf = G.dev<int>(o_rkf); A.ref_feat = G.dev<int>(o_rfeat);
        }
        if (sim3) { A.sim3_before = G.dev<double>(o_a); A.sim3_after = G.dev<double>(o_b); }
        else { A.Tcw_after = G.dev<float>(o_a); A.Ow_after = G.dev<float>(o_b); }
        A.kf = G.dev<MptCorrectKf>(o_view); A.cam_new = G.dev<float>(o_cam);
        A.pos = G.dev<float>(o_pos); A.normal = G.dev<float>(o_nrm); A.min_dist = G.dev<float>(o_min); A.max_dist = G.dev<float>(o_max);
        mpt_launch_correct(c->stream, A, t->T);
        CCM_HIP(c, hipGetLastError());
        // ---- the handles' host copies, brought to the bits the device writes
        for (int k = 0; k < n_moved; k++) {
            ccm_frame* f = u->kfs[k];
            if (sim3) {
                double pose7[7];
                correct_pose7(u->sim3_after + 8 * (size_t)k, pose7);
                ba_pose_to_camera(pose7, f->cam.Tcw, f->cam.Ow);
            } else {
                std::memcpy(f->cam.Tcw, u->Tcw_after + 12 * (size_t)k, 48); std::memcpy(f->cam.Ow, u->Ow_after + 3 * (size_t)k, 12);
            }
            f->has_pose = true;
        }
        if (n == 0 || (!u->pos_out && !u->normal_out && !u->min_dist_out && !u->max_dist_out)) return CCM_OK;
        if ((rc = G.download(c, 0, res_end)) || (rc = G.wait(c))) return rc;
        synced = true;
        G.get(u->pos_out, o_pos, m * 12); G.get(u->normal_out, o_nrm, m * 12);
        G.get(u->min_dist_out, o_min, m * 4); G.get(u->max_dist_out, o_max, m * 4);
        return CCM_OK;
    }, &synced);
}
