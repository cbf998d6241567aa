// mpt_host.cpp -- C ABI of the map-point table (include/ccm_hot.h "map-point table"): the client's map points in device memory,
// created once, updated and fetched by rows at keyframe rate, and refreshed from keyframe handles (ccm_map_table_refresh).  Every
// call stages through the frame handles' block: update [ slot | the given columns ] up, fetch [ columns ] down and [ slot ] up.
#include "mpt_internal.h"
#include <cstddef>
#include <memory>

// The handle gives its reference to the rows back: per-handle memory goes now, the rows with their last handle.  A write of c's that
// is still pending was waited for by the caller (ccm_destroy) or stays recorded in the rows' event (ccm_map_table_destroy).
static void table_release(ccm_map_table* t, bool ctx_going)
{
    if (!t->rows) return;
    {
        std::unique_lock<std::shared_mutex> lk(t->rows->mu);
        if (ctx_going && t->rows->writer == t->ctx) t->rows->writer = nullptr;     // ccm_destroy has waited for the stream
        t->rows->handles--;
    }
    t->rows.reset();                             // hipFree waits for the work still queued on the columns
}

void mpt_tables_orphan(FrameState* S)            // ccm_destroy: the memory goes, the handles stay for ccm_map_table_destroy
{
    for (ccm_map_table* t : S->tables) {
        const int cap = t->capacity;
        table_release(t, true);
        *t = ccm_map_table();
        t->capacity = cap;
    }
    S->tables.clear();
}

extern "C" {

int ccm_map_table_create(ccm_ctx* c, int capacity, ccm_map_table** out)
{
    RoctxRange roctx_("ccm_map_table_create");
    if (out) *out = nullptr;
    if (!c || !out) return CCM_E_ARG;
    if (capacity < 1) return ccm_fail(c, CCM_E_ARG, "map-point table capacity %d < 1", capacity);
    return ccm_guard(c, "ccm_map_table_create", [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        FrameState& S = *frame_state(c);
        const size_t m = (size_t)capacity;
        size_t off = 0;
        const size_t o_pos = seg(off, m * 12), o_nrm = seg(off, m * 12), o_min = seg(off, m * 4), o_max = seg(off, m * 4);
        const size_t o_desc = seg(off, m * 32), o_flags = seg(off, m), o_seen = seg(off, m * 4);
        std::unique_ptr<ccm_map_table> t(new ccm_map_table());
        std::shared_ptr<MptRows> R = std::make_shared<MptRows>();
        if (R->mem.reserve(off)) return ccm_fail(c, CCM_E_NOMEM, "map-point table: device alloc of %zu bytes failed", off);
        uint8_t* b = R->mem.as<uint8_t>();
        if (hipMemsetAsync(b, 0, off, c->stream) != hipSuccess) { (void)hipGetLastError(); return ccm_fail(c, CCM_E_DEVICE, "map-point table: clearing failed"); }
        R->device = c->device; R->capacity = capacity; R->handles = 1;
        R->T = MptTable{ capacity, (float*)(b + o_pos), (float*)(b + o_nrm), (float*)(b + o_min), (float*)(b + o_max), b + o_desc, b + o_flags,
                         (int*)(b + o_seen) };
        t->ctx = c; t->capacity = capacity; t->T = R->T; t->rows = std::move(R);
        S.tables.push_back(t.get());
        *out = t.release();
        return CCM_OK;
    });
}

// A further handle on the rows of `table`, with scratch of its own.  Called on c's thread; of the other context it reads nothing.
int ccm_map_table_attach(ccm_ctx* c, ccm_map_table* table, ccm_map_table** view)
{
    RoctxRange roctx_("ccm_map_table_attach");
    if (view) *view = nullptr;
    if (!c || !table || !view) return CCM_E_ARG;
    if (!table->ctx || !table->rows) return ccm_fail(c, CCM_E_STATE, "ccm_map_table_attach: the table outlived its context");
    return ccm_guard(c, "ccm_map_table_attach", [&]() -> int {
        std::shared_ptr<MptRows> R = table->rows;
        if (R->device != c->device) return ccm_fail(c, CCM_E_ARG, "ccm_map_table_attach: the table lies on device %d, the context on %d", R->device, c->device);
        CCM_HIP(c, hipSetDevice(c->device));
        FrameState& S = *frame_state(c);
        std::unique_ptr<ccm_map_table> t(new ccm_map_table());
        const size_t seen_bytes = (size_t)R->capacity * 4;
        CCM_RESERVE(c, t->seen_mem, seen_bytes);
        CCM_HIP(c, hipMemsetAsync(t->seen_mem.p, 0, seen_bytes, c->stream));
        t->ctx = c; t->capacity = R->capacity; t->T = R->T; t->T.seen = t->seen_mem.as<int>();
        {
            // Writes made while the rows had one handle recorded no event: the first further handle waits for the device once, and
            // every write after it finds two handles (the count changes under the exclusive lock the writers hold)
            std::unique_lock<std::shared_mutex> lk(R->mu);
            if (R->handles.load() == 1) CCM_HIP(c, hipDeviceSynchronize());
            R->handles++;
        }
        t->rows = std::move(R);
        S.tables.push_back(t.get());
        *view = t.release();
        return CCM_OK;
    });
}

int ccm_map_table_handles(const ccm_map_table* t) { return !t ? CCM_E_ARG : t->rows ? t->rows->handles.load() : 0; }

void ccm_map_table_destroy(ccm_map_table* t)
{
    if (!t) return;
    try {
        if (t->ctx && t->ctx->frame) {
            std::vector<ccm_map_table*>& v = t->ctx->frame->tables;
            v.erase(std::remove(v.begin(), v.end(), t), v.end());
            (void)hipSetDevice(t->ctx->device);
        }
        table_release(t, false);
        delete t;                                // hipFree waits for the work still queued on the handle's own columns
    } catch (...) {}
}

int ccm_map_table_capacity(const ccm_map_table* t) { return t ? t->capacity : CCM_E_ARG; }

int ccm_map_table_update(ccm_ctx* c, ccm_map_table* t, const ccm_map_update* u)
{
    RoctxRange roctx_("ccm_map_table_update");
    if (!c || !t || !u) return CCM_E_ARG;
    int rc = check_table(c, t);
    if (rc) return rc;
    if (u->n < 0 || (u->n > 0 && !u->slot)) return ccm_fail(c, CCM_E_ARG, "bad map-point update (n < 0 or no slot list)");
    if (u->n == 0) return CCM_OK;
    return table_call(c, t, true, "ccm_map_table_update", [&]() -> int {         // writes rows and returns with the scatter queued
        const size_t n = (size_t)u->n;
        bool dup = false;
        if ((rc = mark_slots(c, t, u->n, u->slot, &dup))) return rc;
        CCM_HIP(c, hipSetDevice(c->device));
        size_t off = 0;
        const size_t o_slot = seg(off, n * 4), o_pos = seg(off, u->pos ? n * 12 : 0), o_nrm = seg(off, u->normal ? n * 12 : 0);
        const size_t o_min = seg(off, u->min_dist ? n * 4 : 0), o_max = seg(off, u->max_dist ? n * 4 : 0);
        const size_t o_desc = seg(off, u->desc ? n * 32 : 0), o_flags = seg(off, u->flags ? n : 0);
        const size_t end = off;
        Staging& G = frame_state(c)->stage;
        if ((rc = G.reserve(c, end))) return rc;
        int32_t* hs = G.host<int32_t>(o_slot);
        std::memcpy(hs, u->slot, n * 4);
        if (dup) for (int r = 0; r < u->n; r++) if (t->row[u->slot[r]] != r) hs[r] = -1;      // the last row of a slot wins
        G.put(o_pos, u->pos, n * 12); G.put(o_nrm, u->normal, n * 12);
        G.put(o_min, u->min_dist, n * 4); G.put(o_max, u->max_dist, n * 4);
        G.put(o_desc, u->desc, n * 32); G.put(o_flags, u->flags, n);
        if ((rc = G.upload(c, 0, end))) return rc;
        mpt_launch_scatter(c->stream, t->T, u->n, G.dev<int>(o_slot), u->pos ? G.dev<float>(o_pos) : nullptr,
                           u->normal ? G.dev<float>(o_nrm) : nullptr, u->min_dist ? G.dev<float>(o_min) : nullptr,
                           u->max_dist ? G.dev<float>(o_max) : nullptr, u->desc ? G.dev<uint8_t>(o_desc) : nullptr,
                           u->flags ? G.dev<uint8_t>(o_flags) : nullptr);
        CCM_HIP(c, hipGetLastError());
        return CCM_OK;
    });
}

int ccm_map_table_set_order(ccm_ctx* c, ccm_map_table* t, int n, const int32_t* slots)
{
    RoctxRange roctx_("ccm_map_table_set_order");
    if (!c || !t) return CCM_E_ARG;
    int rc = check_table(c, t);
    if (rc) return rc;
    if (!slots) { t->order_all = true; t->n_order = 0; return CCM_OK; }
    if (n < 0) return ccm_fail(c, CCM_E_ARG, "order of %d entries", n);
    return ccm_guard(c, "ccm_map_table_set_order", [&]() -> int {
        bool dup = false;
        if ((rc = mark_slots(c, t, n, slots, &dup))) return rc;
        if (dup) return ccm_fail(c, CCM_E_ARG, "a slot occurs twice in the order");
        CCM_HIP(c, hipSetDevice(c->device));
        if (n > 0) {
            Staging& G = frame_state(c)->stage;
            if ((rc = G.reserve(c, (size_t)n * 4))) return rc;
            G.put(0, slots, (size_t)n * 4);
            CCM_RESERVE(c, t->order, (size_t)n * 4);
            if ((rc = G.upload(c, 0, (size_t)n * 4, t->order.p))) return rc;
        }
        t->order_all = false; t->n_order = n;
        return CCM_OK;
    });
}

int ccm_map_table_fetch(ccm_ctx* c, ccm_map_table* t, int n, const int32_t* slot, float* pos, float* normal, float* min_dist,
                        float* max_dist, uint8_t* desc, uint8_t* flags, int32_t* seen)
{
    if (!c || !t) return CCM_E_ARG;
    int rc = check_table(c, t);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !slot)) return ccm_fail(c, CCM_E_ARG, "bad fetch arguments");
    if (n == 0) return CCM_OK;
    return table_call(c, t, false, "ccm_map_table_fetch", [&]() -> int {
        for (int r = 0; r < n; r++)
            if (slot[r] < 0 || slot[r] >= t->capacity) return ccm_fail(c, CCM_E_ARG, "slot %d (entry %d) outside [0, %d)", slot[r], r, t->capacity);
        CCM_HIP(c, hipSetDevice(c->device));
        const size_t m = (size_t)n;
        size_t off = 0;
        const size_t o_pos = seg(off, m * 12), o_nrm = seg(off, m * 12), o_min = seg(off, m * 4), o_max = seg(off, m * 4);
        const size_t o_desc = seg(off, m * 32), o_flags = seg(off, m), o_seen = seg(off, m * 4);
        const size_t res_end = off;
        const size_t o_slot = seg(off, m * 4);
        Staging& G = frame_state(c)->stage;
        if ((rc = G.reserve(c, off))) return rc;
        G.put(o_slot, slot, m * 4);
        if ((rc = G.upload(c, o_slot, off))) return rc;
        mpt_launch_gather(c->stream, t->T, n, G.dev<int>(o_slot), G.dev<float>(o_pos), G.dev<float>(o_nrm), G.dev<float>(o_min),
                          G.dev<float>(o_max), G.dev<uint8_t>(o_desc), G.dev<uint8_t>(o_flags), G.dev<int>(o_seen));
        CCM_HIP(c, hipGetLastError());
        if ((rc = G.download(c, 0, res_end)) || (rc = G.wait(c))) return rc;
        G.get(pos, o_pos, m * 12); G.get(normal, o_nrm, m * 12);
        G.get(min_dist, o_min, m * 4); G.get(max_dist, o_max, m * 4);
        G.get(desc, o_desc, m * 32); G.get(flags, o_flags, m); G.get(seen, o_seen, m * 4);
        return CCM_OK;
    });
}

// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:929-994) and MapPoint::UpdateNormalAndDepth (:779-823) on keyframe
// handles.  Staging: [ best | normal | min_dist | max_dist ] down, [ slot | obs_first | obs_kf | obs_feat | ref_kf | ref_feat | pos |
// flags | views ] up.  Everything is checked before the staging area is touched.
int ccm_map_table_refresh(ccm_ctx* c, ccm_map_table* t, const ccm_map_refresh* u, ccm_map_refresh_result* res)
{
    RoctxRange roctx_("ccm_map_table_refresh");
    if (!c || !t || !u) return CCM_E_ARG;
    const char* fn = "ccm_map_table_refresh";
    int rc = check_table(c, t);
    if (rc) return rc;
    if (u->n < 0) return ccm_fail(c, CCM_E_ARG, "%s: n = %d", fn, u->n);
    if (u->what == 0 || (u->what & ~(CCM_MPR_DESCRIPTOR | CCM_MPR_NORMAL_DEPTH))) return ccm_fail(c, CCM_E_ARG, "%s: what = %d", fn, u->what);
    const bool nd = (u->what & CCM_MPR_NORMAL_DEPTH) != 0;
    if (u->n_kf < 0 || (u->n_kf > 0 && !u->kfs)) return ccm_fail(c, CCM_E_ARG, "%s: n_kf = %d%s", fn, u->n_kf, u->n_kf > 0 ? " and null kfs" : "");
    if (u->n > 0 && (!u->slot || !u->obs_first || (nd && (!u->ref_kf || !u->ref_feat))))
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !u->slot ? "slot" : !u->obs_first ? "obs_first" : !u->ref_kf ? "ref_kf" : "ref_feat");
    if (u->n == 0) return CCM_OK;
    bool synced = false;                                                       // writes rows; with a result it waits for them
    return table_call(c, t, true, fn, [&]() -> int {
        const int n = u->n, n_kf = u->n_kf;
        if (u->obs_first[0] != 0) return ccm_fail(c, CCM_E_ARG, "%s: obs_first[0] = %d, not 0", fn, u->obs_first[0]);
        for (int p = 0; p < n; p++)
            if (u->obs_first[p + 1] < u->obs_first[p])
                return ccm_fail(c, CCM_E_ARG, "%s: obs_first[%d] = %d below obs_first[%d] = %d", fn, p + 1, u->obs_first[p + 1], p, u->obs_first[p]);
        const int n_obs = u->obs_first[n];
        if (n_obs > 0 && (!u->obs_kf || !u->obs_feat)) return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !u->obs_kf ? "obs_kf" : "obs_feat");
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* f = u->kfs[k];
            if (!f) return ccm_fail(c, CCM_E_ARG, "%s: null kfs[%d]", fn, k);
            if ((rc = frame_named_check(c, f, CCM_E_STATE, fn, "kfs[%d]", k))) return rc;
        }
        std::vector<uint8_t> used((size_t)n_kf, 0);              // 1: named by an observation, 2: named as a reference keyframe
        for (int p = 0; p < n; p++) {
            for (int e = u->obs_first[p]; e < u->obs_first[p + 1]; e++) {
                const int k = u->obs_kf[e];
                if (k < 0 || k >= n_kf) return ccm_fail(c, CCM_E_ARG, "%s: point %d, entry %d: keyframe %d outside [0, %d)", fn, p, e, k, n_kf);
                if (u->obs_feat[e] < 0 || u->obs_feat[e] >= u->kfs[k]->n)
                    return ccm_fail(c, CCM_E_ARG, "%s: point %d, entry %d: feature %d outside [0, %d) of kfs[%d]", fn, p, e, u->obs_feat[e], u->kfs[k]->n, k);
                used[k] |= 1;
            }
            if (nd && u->obs_first[p + 1] > u->obs_first[p]) {
                const int k = u->ref_kf[p];
                if (k < 0 || k >= n_kf) return ccm_fail(c, CCM_E_ARG, "%s: point %d: reference keyframe %d outside [0, %d)", fn, p, k, n_kf);
                if (u->ref_feat[p] < 0 || u->ref_feat[p] >= u->kfs[k]->n)
                    return ccm_fail(c, CCM_E_ARG, "%s: point %d: reference feature %d outside [0, %d) of kfs[%d]", fn, p, u->ref_feat[p], u->kfs[k]->n, k);
                used[k] |= 2;
            }
        }
        if (nd)
            for (int k = 0; k < n_kf; k++) {
                const ccm_frame* f = u->kfs[k];
                if ((used[k] & 1) && !f->has_pose) return ccm_fail(c, CCM_E_STATE, "%s: kfs[%d] is observed and has no pose", fn, k);
                if ((used[k] & 2) && (!f->has_pose || !f->has_cam))
                    return ccm_fail(c, CCM_E_STATE, "%s: kfs[%d] is a reference keyframe and has no %s", fn, k, !f->has_pose ? "pose" : "camera");
            }
        bool dup = false;
        if ((rc = mark_slots(c, t, n, u->slot, &dup))) return rc;
        if (dup) return ccm_fail(c, CCM_E_ARG, "%s: a slot is listed twice", fn);

        CCM_HIP(c, hipSetDevice(c->device));
        const size_t m = (size_t)n, mo = (size_t)n_obs;
        size_t off = 0;
        const size_t o_best = seg(off, m * 4), o_nrm = seg(off, m * 12), o_min = seg(off, m * 4), o_max = seg(off, m * 4);
        const size_t res_end = off;
        const size_t o_slot = seg(off, m * 4), o_first = seg(off, (m + 1) * 4), o_okf = seg(off, mo * 4), o_ofeat = seg(off, mo * 4);
        const size_t o_rkf = seg(off, nd ? m * 4 : 0), o_rfeat = seg(off, nd ? m * 4 : 0);
        const size_t o_pos = seg(off, u->pos ? m * 12 : 0), o_flags = seg(off, u->flags ? m : 0);
        const size_t o_view = seg(off, (size_t)n_kf * sizeof(MptKfView));
        const size_t end = off;
        Staging& G = frame_state(c)->stage;
        if ((rc = G.reserve(c, end))) return rc;
        G.put(o_slot, u->slot, m * 4); G.put(o_first, u->obs_first, (m + 1) * 4);
        G.put(o_okf, u->obs_kf, mo * 4); G.put(o_ofeat, u->obs_feat, mo * 4);
        if (nd) {
            int32_t* rk = G.host<int32_t>(o_rkf); int32_t* rf = G.host<int32_t>(o_rfeat);
            for (int p = 0; p < n; p++) {                        // not read for a point without observations: any value the caller left
                const bool has = u->obs_first[p + 1] > u->obs_first[p];
                rk[p] = has ? u->ref_kf[p] : 0; rf[p] = has ? u->ref_feat[p] : 0;
            }
        }
        G.put(o_pos, u->pos, m * 12); G.put(o_flags, u->flags, m);
        MptKfView* hv = G.host<MptKfView>(o_view);
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* f = u->kfs[k];
            hv[k] = MptKfView{ f->desc, f->d_cam ? (const float*)((const uint8_t*)f->d_cam + offsetof(MapCam, Ow)) : nullptr, f->oct, f->sf, f->cam_levels, 0 };
        }
        if ((rc = G.upload(c, o_slot, end))) return rc;
        MptRefreshArgs A{};
        A.n = n; A.what = u->what;
        A.slot = G.dev<int>(o_slot); A.obs_first = G.dev<int>(o_first); A.obs_kf = G.dev<int>(o_okf);
        A.obs_feat = G.dev<int>(o_ofeat); A.ref_kf = G.dev<int>(o_rkf); A.ref_feat = G.dev<int>(o_rfeat);
        A.pos = u->pos ? G.dev<float>(o_pos) : nullptr; A.flags = u->flags ? G.dev<uint8_t>(o_flags) : nullptr;
        A.view = G.dev<MptKfView>(o_view);
        A.best = G.dev<int>(o_best); A.normal = G.dev<float>(o_nrm); A.min_dist = G.dev<float>(o_min); A.max_dist = G.dev<float>(o_max);
        mpt_launch_refresh(c->stream, A, t->T);
        CCM_HIP(c, hipGetLastError());
        if (!res || (!res->best && !res->normal && !res->min_dist && !res->max_dist)) return CCM_OK;
        if ((rc = G.download(c, 0, res_end)) || (rc = G.wait(c))) return rc;
        synced = true;
        G.get(res->best, o_best, m * 4); G.get(res->normal, o_nrm, m * 12);
        G.get(res->min_dist, o_min, m * 4); G.get(res->max_dist, o_max, m * 4);
        return CCM_OK;
    }, &synced);
}

}  // extern "C"
