// mpt_host.cpp -- C ABI of the map-point table (include/ccm_hot.h "map-point table"): the client's map points in device memory,
// updated by rows at keyframe rate, and the two per-frame calls of Tracking::TrackLocalMap that work on a frame handle and the
// table: SearchLocalPoints (src/Tracking.cpp:860-922) and PoseOptimizationClient (src/Optimizer.cpp:215-347); and
// TrackWithMotionModel (src/Tracking.cpp:569-621) on two frame handles and the table, at the end of this file.
//
// The calls share the frame handles' page-locked staging area and its device twin `io` (frame_internal.h).  SearchLocalPoints
// uploads nothing: its parameters travel as kernel arguments.  Its result block is
//   [ status | match | occupied | mp_id | count | in-view slots | proj_x | proj_y | level | view_cos ]
// of which the first download takes everything up to the count, and the second, behind the matcher, the first four segments again;
// the slot list and the taps are copied at their exact length once the count is known and land with the second download.
#include "frame_internal.h"
#include "mpt_types.h"
#include <chrono>
#include <climits>
#include <cstddef>

struct ccm_map_table {
    ccm_ctx* ctx = nullptr;                      // nullptr once the context is gone
    int capacity = 0;
    DevBuf mem;                                  // the columns, one block
    MptTable T{};
    DevBuf order; int n_order = 0; bool order_all = true;    // order_all: ascending slot over the LIVE slots
    int stamp = 0;                               // per-table call counter of SearchLocalPoints: seen[slot] == stamp <=> seen in this call
    std::vector<uint32_t> gen; std::vector<int32_t> row; uint32_t cur_gen = 0;   // host: last row of a slot within one update / order
    DevBuf where; unsigned fuse_stamp = 0;       // ccm_fuse_select_table_frames: per slot, stamp << 32 | position in that call's slot list
};

void mpt_tables_orphan(FrameState* S)            // ccm_destroy: the memory goes, the handles stay for ccm_map_table_destroy
{
    for (ccm_map_table* t : S->tables) {
        const int cap = t->capacity;
        *t = ccm_map_table();
        t->capacity = cap;
    }
    S->tables.clear();
}

static int check_table(ccm_ctx* c, const ccm_map_table* t)
{
    if (!t->ctx) return ccm_fail(c, CCM_E_STATE, "map-point table outlived its context");
    if (t->ctx != c) return ccm_fail(c, CCM_E_ARG, "map-point table belongs to another context");
    return CCM_OK;
}

// Marks every slot of list [n] with its last position; CCM_E_ARG for a slot outside the table.  dup: whether a slot occurs twice.
static int mark_slots(ccm_ctx* c, ccm_map_table* t, int n, const int32_t* list, bool* dup)
{
    for (int r = 0; r < n; r++)
        if (list[r] < 0 || list[r] >= t->capacity) return ccm_fail(c, CCM_E_ARG, "slot %d (entry %d) outside [0, %d)", list[r], r, t->capacity);
    if (t->gen.empty()) { t->gen.assign(t->capacity, 0); t->row.assign(t->capacity, 0); }
    if (++t->cur_gen == 0) { std::fill(t->gen.begin(), t->gen.end(), 0); t->cur_gen = 1; }
    *dup = false;
    for (int r = 0; r < n; r++) {
        const int s = list[r];
        if (t->gen[s] == t->cur_gen) *dup = true;
        t->gen[s] = t->cur_gen; t->row[s] = r;
    }
    return CCM_OK;
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
        ccm_map_table* t = new ccm_map_table();
        if (t->mem.reserve(off)) { delete t; return ccm_fail(c, CCM_E_NOMEM, "map-point table: device alloc of %zu bytes failed", off); }
        uint8_t* b = t->mem.as<uint8_t>();
        if (hipMemsetAsync(b, 0, off, c->stream) != hipSuccess) { (void)hipGetLastError(); delete t; return ccm_fail(c, CCM_E_DEVICE, "map-point table: clearing failed"); }
        t->ctx = c; t->capacity = capacity;
        t->T = MptTable{ capacity, (float*)(b + o_pos), (float*)(b + o_nrm), (float*)(b + o_min), (float*)(b + o_max), b + o_desc, b + o_flags,
                         (int*)(b + o_seen) };
        S.tables.push_back(t);
        *out = t;
        return CCM_OK;
    });
}

void ccm_map_table_destroy(ccm_map_table* t)
{
    if (!t) return;
    try {
        if (t->ctx && t->ctx->frame) {
            std::vector<ccm_map_table*>& v = t->ctx->frame->tables;
            v.erase(std::remove(v.begin(), v.end(), t), v.end());
            (void)hipSetDevice(t->ctx->device);
        }
        delete t;                                // hipFree waits for the work still queued on the columns
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
    return ccm_guard(c, "ccm_map_table_update", [&]() -> int {
        const size_t n = (size_t)u->n;
        bool dup = false;
        if ((rc = mark_slots(c, t, u->n, u->slot, &dup))) return rc;
        CCM_HIP(c, hipSetDevice(c->device));
        size_t off = 0;
        const size_t o_slot = seg(off, n * 4), o_pos = seg(off, u->pos ? n * 12 : 0), o_nrm = seg(off, u->normal ? n * 12 : 0);
        const size_t o_min = seg(off, u->min_dist ? n * 4 : 0), o_max = seg(off, u->max_dist ? n * 4 : 0);
        const size_t o_desc = seg(off, u->desc ? n * 32 : 0), o_flags = seg(off, u->flags ? n : 0);
        const size_t end = off;
        uint8_t* h = nullptr;
        if ((rc = frame_staging(c, end, &h))) return rc;
        int32_t* hs = (int32_t*)(h + o_slot);
        std::memcpy(hs, u->slot, n * 4);
        if (dup) for (int r = 0; r < u->n; r++) if (t->row[u->slot[r]] != r) hs[r] = -1;      // the last row of a slot wins
        if (u->pos) std::memcpy(h + o_pos, u->pos, n * 12);
        if (u->normal) std::memcpy(h + o_nrm, u->normal, n * 12);
        if (u->min_dist) std::memcpy(h + o_min, u->min_dist, n * 4);
        if (u->max_dist) std::memcpy(h + o_max, u->max_dist, n * 4);
        if (u->desc) std::memcpy(h + o_desc, u->desc, n * 32);
        if (u->flags) std::memcpy(h + o_flags, u->flags, n);
        if ((rc = frame_upload(c, 0, end))) return rc;
        const uint8_t* io = frame_state(c)->io.as<uint8_t>();
        mpt_launch_scatter(c->stream, t->T, u->n, (const int*)(io + o_slot), u->pos ? (const float*)(io + o_pos) : nullptr,
                           u->normal ? (const float*)(io + o_nrm) : nullptr, u->min_dist ? (const float*)(io + o_min) : nullptr,
                           u->max_dist ? (const float*)(io + o_max) : nullptr, u->desc ? io + o_desc : nullptr, u->flags ? io + o_flags : nullptr);
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
            uint8_t* h = nullptr;
            if ((rc = frame_staging(c, (size_t)n * 4, &h))) return rc;
            std::memcpy(h, slots, (size_t)n * 4);
            CCM_RESERVE(c, t->order, (size_t)n * 4);
            if ((rc = frame_upload(c, 0, (size_t)n * 4, t->order.p))) return rc;
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
    return ccm_guard(c, "ccm_map_table_fetch", [&]() -> int {
        for (int r = 0; r < n; r++)
            if (slot[r] < 0 || slot[r] >= t->capacity) return ccm_fail(c, CCM_E_ARG, "slot %d (entry %d) outside [0, %d)", slot[r], r, t->capacity);
        CCM_HIP(c, hipSetDevice(c->device));
        const size_t m = (size_t)n;
        size_t off = 0;
        const size_t o_pos = seg(off, m * 12), o_nrm = seg(off, m * 12), o_min = seg(off, m * 4), o_max = seg(off, m * 4);
        const size_t o_desc = seg(off, m * 32), o_flags = seg(off, m), o_seen = seg(off, m * 4);
        const size_t res_end = off;
        const size_t o_slot = seg(off, m * 4);
        uint8_t* h = nullptr;
        if ((rc = frame_staging(c, off, &h))) return rc;
        std::memcpy(h + o_slot, slot, m * 4);
        if ((rc = frame_upload(c, o_slot, off))) return rc;
        uint8_t* io = frame_state(c)->io.as<uint8_t>();
        mpt_launch_gather(c->stream, t->T, n, (const int*)(io + o_slot), (float*)(io + o_pos), (float*)(io + o_nrm), (float*)(io + o_min),
                          (float*)(io + o_max), io + o_desc, io + o_flags, (int*)(io + o_seen));
        CCM_HIP(c, hipGetLastError());
        if ((rc = frame_download(c, res_end))) return rc;
        if (pos) std::memcpy(pos, h + o_pos, m * 12);
        if (normal) std::memcpy(normal, h + o_nrm, m * 12);
        if (min_dist) std::memcpy(min_dist, h + o_min, m * 4);
        if (max_dist) std::memcpy(max_dist, h + o_max, m * 4);
        if (desc) std::memcpy(desc, h + o_desc, m * 32);
        if (flags) std::memcpy(flags, h + o_flags, m);
        if (seen) std::memcpy(seen, h + o_seen, m * 4);
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
    return ccm_guard(c, fn, [&]() -> int {
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
            if ((rc = frame_named_check(c, f, fn, "kfs[%d]", k))) return rc;
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
        uint8_t* h = nullptr;
        if ((rc = frame_staging(c, end, &h))) return rc;
        std::memcpy(h + o_slot, u->slot, m * 4); std::memcpy(h + o_first, u->obs_first, (m + 1) * 4);
        if (mo) { std::memcpy(h + o_okf, u->obs_kf, mo * 4); std::memcpy(h + o_ofeat, u->obs_feat, mo * 4); }
        if (nd) {
            int32_t* rk = (int32_t*)(h + o_rkf); int32_t* rf = (int32_t*)(h + o_rfeat);
            for (int p = 0; p < n; p++) {                        // not read for a point without observations: any value the caller left
                const bool has = u->obs_first[p + 1] > u->obs_first[p];
                rk[p] = has ? u->ref_kf[p] : 0; rf[p] = has ? u->ref_feat[p] : 0;
            }
        }
        if (u->pos) std::memcpy(h + o_pos, u->pos, m * 12);
        if (u->flags) std::memcpy(h + o_flags, u->flags, m);
        MptKfView* hv = (MptKfView*)(h + o_view);
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* f = u->kfs[k];
            hv[k] = MptKfView{ f->desc, f->d_cam ? (const float*)((const uint8_t*)f->d_cam + offsetof(MapCam, Ow)) : nullptr, f->oct, f->sf, f->cam_levels, 0 };
        }
        if ((rc = frame_upload(c, o_slot, end))) return rc;
        uint8_t* io = frame_state(c)->io.as<uint8_t>();
        MptRefreshArgs A{};
        A.n = n; A.what = u->what;
        A.slot = (const int*)(io + o_slot); A.obs_first = (const int*)(io + o_first); A.obs_kf = (const int*)(io + o_okf);
        A.obs_feat = (const int*)(io + o_ofeat); A.ref_kf = (const int*)(io + o_rkf); A.ref_feat = (const int*)(io + o_rfeat);
        A.pos = u->pos ? (const float*)(io + o_pos) : nullptr; A.flags = u->flags ? io + o_flags : nullptr;
        A.view = (const MptKfView*)(io + o_view);
        A.best = (int*)(io + o_best); A.normal = (float*)(io + o_nrm); A.min_dist = (float*)(io + o_min); A.max_dist = (float*)(io + o_max);
        mpt_launch_refresh(c->stream, A, t->T);
        CCM_HIP(c, hipGetLastError());
        if (!res || (!res->best && !res->normal && !res->min_dist && !res->max_dist)) return CCM_OK;
        if ((rc = frame_download(c, res_end))) return rc;
        if (res->best) std::memcpy(res->best, h + o_best, m * 4);
        if (res->normal) std::memcpy(res->normal, h + o_nrm, m * 12);
        if (res->min_dist) std::memcpy(res->min_dist, h + o_min, m * 4);
        if (res->max_dist) std::memcpy(res->max_dist, h + o_max, m * 4);
        return CCM_OK;
    });
}

// what a keyframe costs in the staging copy of ccm_fuse_select_table_frames (tools/bench_fuse_table.py counts the upload with these)
static_assert(sizeof(FuseView) == 112 && sizeof(WinGrid) == 80, "per-keyframe upload of ccm_fuse_select_table_frames");

// ORBmatcher::Fuse, both overloads (src/ORBmatcher.cpp:854-1000, :1002-1122), up to the selection, for every (keyframe, point) pair.
// Staging: [ count | best_idx | best_dist | gate | u | v | level ] down, [ views | grids | slot | skip | inv_level_sigma2 ] up; the
// taps take room only when asked for.  The query list and the selections stay in device memory (FrameState::fuse).
int ccm_fuse_select_table_frames(ccm_ctx* c, ccm_map_table* t, const ccm_fuse_table_problem* p, ccm_fuse_table_result* r)
{
    RoctxRange roctx_("ccm_fuse_select_table_frames");
    if (!c || !t || !p || !r) return CCM_E_ARG;
    const char* fn = "ccm_fuse_select_table_frames";
    int rc = check_table(c, t);
    if (rc) return rc;
    if (p->n_kf < 0 || p->n_points < 0) return ccm_fail(c, CCM_E_ARG, "%s: n_kf = %d, n_points = %d", fn, p->n_kf, p->n_points);
    if (p->n_kf == 0 || p->n_points == 0) { r->n_searched = 0; return CCM_OK; }
    if (!p->views || !p->slot || !p->scale_factors || !r->best_idx || (p->chi2_check && !p->inv_level_sigma2))
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !p->views ? "views" : !p->slot ? "slot" : !p->scale_factors ? "scale_factors" :
                        !r->best_idx ? "best_idx" : "inv_level_sigma2 with chi2_check");
    if (p->n_levels < 1 || p->n_levels > CCM_MAX_LEVELS) return ccm_fail(c, CCM_E_ARG, "%s: n_levels = %d outside 1..%d", fn, p->n_levels, CCM_MAX_LEVELS);
    if ((r->u || r->v || r->level) && !(r->u && r->v && r->level)) return ccm_fail(c, CCM_E_ARG, "%s: the taps u, v and level come together", fn);
    if (p->n_kf > 65535 || (size_t)p->n_kf * (size_t)p->n_points > ((size_t)1 << 24))
        return ccm_fail(c, CCM_E_CAPACITY, "%s: %d keyframes x %d points; at most 65535 keyframes and 2^24 pairs a call", fn, p->n_kf, p->n_points);
    return ccm_guard(c, fn, [&]() -> int {
        const int n_kf = p->n_kf, n_pt = p->n_points;
        int max_n = 0;
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* f = p->views[k].kf;
            if (!f) return ccm_fail(c, CCM_E_ARG, "%s: null views[%d].kf", fn, k);
            if ((rc = frame_named_check(c, f, fn, "views[%d].kf", k))) return rc;
            max_n = std::max(max_n, f->n);
        }
        bool dup = false;
        if ((rc = mark_slots(c, t, n_pt, p->slot, &dup))) return rc;
        if (dup) return ccm_fail(c, CCM_E_ARG, "%s: a slot is listed twice", fn);

        CCM_HIP(c, hipSetDevice(c->device));
        FrameState& S = *frame_state(c);
        hipStream_t st = c->stream;
        const size_t m = (size_t)n_kf * (size_t)n_pt;
        const bool taps = r->u != nullptr;
        size_t off = 0;
        const size_t o_cnt = seg(off, 16), o_bi = seg(off, m * 4), o_bd = seg(off, r->best_dist ? m * 4 : 0), o_gate = seg(off, r->gate ? m : 0);
        const size_t o_u = seg(off, taps ? m * 4 : 0), o_v = seg(off, taps ? m * 4 : 0), o_lvl = seg(off, taps ? m * 4 : 0);
        const size_t res_end = off;
        const size_t o_view = seg(off, (size_t)n_kf * sizeof(FuseView)), o_grid = seg(off, (size_t)n_kf * sizeof(WinGrid));
        const size_t o_slot = seg(off, (size_t)n_pt * 4), o_skip = seg(off, p->skip ? (size_t)n_pt : 0);
        const size_t o_is2 = seg(off, p->chi2_check ? CCM_MAX_LEVELS * 4 : 0);
        const size_t end = off;
        uint8_t* h = nullptr;
        if ((rc = frame_staging(c, end, &h))) return rc;
        size_t w = 0;                                                          // device-only work area
        const size_t w_held = seg(w, m), w_qx = seg(w, m * 4), w_qy = seg(w, m * 4), w_qr = seg(w, m * 4), w_minl = seg(w, m * 4), w_maxl = seg(w, m * 4);
        const size_t w_qkf = seg(w, m * 4), w_qpair = seg(w, m * 4), w_qdesc = seg(w, m * 32), w_si = seg(w, m * 4), w_sd = seg(w, m * 4);
        CCM_RESERVE(c, S.fuse, w + 64);
        if (!t->where.p) {                                                     // first Fuse on this table: every entry older than any stamp
            CCM_RESERVE(c, t->where, (size_t)t->capacity * 8);
            CCM_HIP(c, hipMemsetAsync(t->where.p, 0, (size_t)t->capacity * 8, st));
            t->fuse_stamp = 0;
        }
        if (t->fuse_stamp == 0xffffffffu) { CCM_HIP(c, hipMemsetAsync(t->where.p, 0, (size_t)t->capacity * 8, st)); t->fuse_stamp = 0; }
        const unsigned stamp = ++t->fuse_stamp;

        FuseView* hv = (FuseView*)(h + o_view); WinGrid* hg = (WinGrid*)(h + o_grid);
        for (int k = 0; k < n_kf; k++) {
            const ccm_fuse_view& V = p->views[k];
            const ccm_frame* f = V.kf;
            FuseView& D = hv[k];
            std::memcpy(D.Tcw, V.Tcw, sizeof D.Tcw); std::memcpy(D.Ow, V.Ow, sizeof D.Ow);
            D.fx = V.fx; D.fy = V.fy; D.cx = V.cx; D.cy = V.cy; D.min_x = V.min_x; D.max_x = V.max_x; D.min_y = V.min_y; D.max_y = V.max_y;
            D.n = f->n; D.pad_ = 0; D.mp_id = f->mp_id;
            hg[k] = frame_win_grid(f);
        }
        std::memcpy(h + o_slot, p->slot, (size_t)n_pt * 4);
        if (p->skip) std::memcpy(h + o_skip, p->skip, (size_t)n_pt);
        if (p->chi2_check) {
            float* is2 = (float*)(h + o_is2);
            for (int l = 0; l < CCM_MAX_LEVELS; l++) is2[l] = l < p->n_levels ? p->inv_level_sigma2[l] : 0.f;
        }
        if ((rc = frame_upload(c, o_view, end))) return rc;
        uint8_t* io = S.io.as<uint8_t>(); uint8_t* wk = S.fuse.as<uint8_t>();
        FuseArgs A{};
        A.n_kf = n_kf; A.n_points = n_pt;
        A.views = (const FuseView*)(io + o_view); A.slot = (const int*)(io + o_slot); A.skip = p->skip ? io + o_skip : nullptr;
        A.where = t->where.as<unsigned long long>(); A.stamp = stamp; A.held = wk + w_held;
        A.log_scale = p->log_scale_factor; A.n_levels = p->n_levels; A.th = p->th;
        for (int l = 0; l < CCM_MAX_LEVELS; l++) A.scale[l] = l < p->n_levels ? p->scale_factors[l] : 0.f;
        A.best_idx = (int*)(io + o_bi); A.best_dist = r->best_dist ? (int*)(io + o_bd) : nullptr; A.gate = r->gate ? io + o_gate : nullptr;
        A.u = taps ? (float*)(io + o_u) : nullptr; A.v = taps ? (float*)(io + o_v) : nullptr; A.level = taps ? (int*)(io + o_lvl) : nullptr;
        A.cnt = (int*)(io + o_cnt); A.qx = (float*)(wk + w_qx); A.qy = (float*)(wk + w_qy); A.qr = (float*)(wk + w_qr);
        A.minl = (int*)(wk + w_minl); A.maxl = (int*)(wk + w_maxl); A.qkf = (int*)(wk + w_qkf); A.qpair = (int*)(wk + w_qpair); A.qdesc = wk + w_qdesc;
        CCM_HIP(c, hipMemsetAsync(A.cnt, 0, 16, st));
        CCM_HIP(c, hipMemsetAsync(A.held, 0, m, st));
        fuse_launch_project(st, A, t->T, max_n);
        CCM_HIP(c, hipGetLastError());
        if ((rc = frame_download(c, 16))) return rc;                           // the number of queries: the first synchronisation
        int nq = 0;
        std::memcpy(&nq, h + o_cnt, 4);
        if (nq < 0 || (size_t)nq > m) return ccm_fail(c, CCM_E_DEVICE, "%s: %d queries of %zu pairs", fn, nq, m);
        if (nq > 0) {
            match_launch_window_select_batch(st, (const WinGrid*)(io + o_grid), A.qkf, nq, A.qx, A.qy, A.qr, A.minl, A.maxl, A.qdesc,
                                             p->chi2_check ? (const float*)(io + o_is2) : nullptr, p->accept_th, (int*)(wk + w_si), (int*)(wk + w_sd));
            fuse_launch_scatter(st, nq, (int)m, A.qpair, (const int*)(wk + w_si), (const int*)(wk + w_sd), A.best_idx, A.best_dist);
            CCM_HIP(c, hipGetLastError());
        }
        if ((rc = frame_download(c, res_end))) return rc;                      // the second
        std::memcpy(r->best_idx, h + o_bi, m * 4);
        if (r->best_dist) std::memcpy(r->best_dist, h + o_bd, m * 4);
        if (r->gate) std::memcpy(r->gate, h + o_gate, m);
        if (taps) { std::memcpy(r->u, h + o_u, m * 4); std::memcpy(r->v, h + o_v, m * 4); std::memcpy(r->level, h + o_lvl, m * 4); }
        r->n_searched = nq;
        return CCM_OK;
    });
}

// Tracking::SearchLocalPoints, src/Tracking.cpp:860-922
int ccm_frame_search_local_points(ccm_ctx* c, ccm_frame* f, ccm_map_table* t, const ccm_slp_params* p, ccm_slp_result* r)
{
    RoctxRange roctx_("ccm_frame_search_local_points");
    if (!c || !f || !t || !p || !r) return CCM_E_ARG;
    int rc = frame_check(c, f);
    if (rc || (rc = check_table(c, t))) return rc;
    if (p->n_levels < 1 || p->n_levels > CCM_MAX_LEVELS || !p->scale_factors || r->in_view_cap < 0 || (r->in_view_cap > 0 && !r->in_view_slot) ||
        (f->n > 0 && (!r->match || !r->mp_id)))
        return ccm_fail(c, CCM_E_ARG, "bad SearchLocalPoints arguments (n_levels in 1..%d, match and mp_id of N entries)", CCM_MAX_LEVELS);
    using clk = std::chrono::steady_clock;
    const clk::time_point t_entry = clk::now();
    clk::time_point t_before, t_after;
    bool timed = false;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const int ret = ccm_guard(c, "ccm_frame_search_local_points", [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        FrameState& S = *frame_state(c);
        hipStream_t st = c->stream;
        const int n = f->n, n_order = t->order_all ? t->capacity : t->n_order, n_wg = slp_workgroups(n_order);
        const size_t m = (size_t)n_order;
        if (t->stamp == INT_MAX) { CCM_HIP(c, hipMemsetAsync(t->T.seen, 0, (size_t)t->capacity * 4, st)); t->stamp = 0; }
        const int stamp = ++t->stamp;

        size_t off = 0;
        const size_t o_status = seg(off, 16), o_out = seg(off, (size_t)n * 4), o_flag = seg(off, (size_t)n), o_ids = seg(off, (size_t)n * 4);
        const size_t res_end = o_ids + (size_t)n * 4;
        const size_t o_cnt = seg(off, 16), o_slots = seg(off, m * 4);
        const size_t first_end = o_cnt + 16;
        const size_t o_px = seg(off, m * 4), o_py = seg(off, m * 4), o_lvl = seg(off, m * 4), o_vc = seg(off, m * 4);
        uint8_t* h = nullptr;
        if ((rc = frame_staging(c, off, &h))) return rc;
        size_t w = 0;                                                          // device-only work area
        const size_t w_u = seg(w, m * 4), w_v = seg(w, m * 4), w_vc = seg(w, m * 4), w_lvl = seg(w, m * 4);
        const size_t w_mask = seg(w, (size_t)n_wg * (SLP_TPB / 64) * 8), w_cnt = seg(w, (size_t)n_wg * 4), w_off = seg(w, (size_t)n_wg * 4);
        const size_t w_qr = seg(w, m * 4), w_minl = seg(w, m * 4), w_maxl = seg(w, m * 4), w_qdesc = seg(w, m * 32);
        const size_t w_act = seg(w, m), w_qflag = seg(w, m);
        CCM_RESERVE(c, S.slp, w + 64);
        uint8_t* io = S.io.as<uint8_t>(); uint8_t* wk = S.slp.as<uint8_t>();
        int* d_cnt = (int*)(io + o_cnt); int* d_ids = (int*)(io + o_ids);

        CCM_HIP(c, hipMemsetAsync(d_cnt, 0, 16, st));
        slp_launch_mark(st, t->T, n, f->mp_id, stamp, d_ids, io + o_flag, (int*)(io + o_out), d_cnt);
        CCM_HIP(c, hipGetLastError());
        SlpArgs A{};
        A.n_order = n_order; A.order = t->order_all ? nullptr : t->order.as<int>(); A.stamp = stamp;
        std::memcpy(A.Tcw, p->Tcw, sizeof A.Tcw); std::memcpy(A.Ow, p->Ow, sizeof A.Ow);
        A.fx = p->fx; A.fy = p->fy; A.cx = p->cx; A.cy = p->cy; A.min_x = p->min_x; A.max_x = p->max_x; A.min_y = p->min_y; A.max_y = p->max_y;
        A.cos_limit = p->viewing_cos_limit; A.log_scale = p->log_scale_factor; A.n_levels = p->n_levels; A.th = p->th;
        for (int l = 0; l < CCM_MAX_LEVELS; l++) A.scale[l] = l < p->n_levels ? p->scale_factors[l] : 0.f;
        A.tmp_u = (float*)(wk + w_u); A.tmp_v = (float*)(wk + w_v); A.tmp_vc = (float*)(wk + w_vc); A.tmp_level = (int*)(wk + w_lvl);
        A.mask = (unsigned long long*)(wk + w_mask); A.wg_cnt = (int*)(wk + w_cnt); A.wg_off = (int*)(wk + w_off);
        A.qx = (float*)(io + o_px); A.qy = (float*)(io + o_py); A.qr = (float*)(wk + w_qr); A.minl = (int*)(wk + w_minl); A.maxl = (int*)(wk + w_maxl);
        A.qdesc = wk + w_qdesc; A.qact = wk + w_act; A.qflag = wk + w_qflag; A.slots = (int*)(io + o_slots);
        A.tap_level = (int*)(io + o_lvl); A.tap_vc = (float*)(io + o_vc);
        slp_launch_frustum(st, A, t->T, d_cnt);
        CCM_HIP(c, hipGetLastError());
        t_before = clk::now();
        if ((rc = frame_download(c, first_end))) return rc;                    // the count (16 bytes) behind the first loop's results
        t_after = clk::now(); timed = true;

        int head[2];
        std::memcpy(head, h + o_cnt, 8);
        const int nv = head[0];
        if (head[1]) return ccm_fail(c, CCM_E_ARG, "the frame holds a map-point id outside [0, %d) or of a slot that is not LIVE", t->capacity);
        if (nv < 0 || nv > n_order) return ccm_fail(c, CCM_E_DEVICE, "%d entries in view of %d", nv, n_order);
        r->n_to_match = nv;
        if (nv > r->in_view_cap) return ccm_fail(c, CCM_E_CAPACITY, "%d map points in view, room for %d", nv, r->in_view_cap);
        if (n > 0) CCM_HIP(c, hipMemcpyAsync(f->mp_id, d_ids, (size_t)n * 4, hipMemcpyDeviceToDevice, st));   // the bad ones cleared
        const bool taps = r->proj_x || r->proj_y || r->level || r->view_cos;
        if (nv == 0 || n == 0) {                                               // :910: no matcher
            for (int i = 0; i < n; i++) r->match[i] = -1;
            if (n > 0) std::memcpy(r->mp_id, h + o_ids, (size_t)n * 4);
            if (n > 0 && r->occupied) std::memcpy(r->occupied, h + o_flag, n);
            if (nv == 0) return 0;
            if ((rc = frame_fetch(c, h + o_slots, io + o_slots, (size_t)nv * 4))) return rc;      // an empty frame: the slot list alone
            if (taps && (rc = frame_fetch(c, h + o_px, io + o_px, (o_vc + (size_t)nv * 4) - o_px))) return rc;
        } else {                                                               // exact lengths; they land before the matcher's download
            CCM_HIP(c, hipMemcpyAsync(h + o_slots, io + o_slots, (size_t)nv * 4, hipMemcpyDeviceToHost, st));
            if (taps)
                for (size_t o : { o_px, o_py, o_lvl, o_vc }) CCM_HIP(c, hipMemcpyAsync(h + o, io + o, (size_t)nv * 4, hipMemcpyDeviceToHost, st));
        }
        int nmatches = 0;
        if (nv > 0 && n > 0) {
            WinDevCall D{ 0, nv, A.qx, A.qy, A.qr, A.minl, A.maxl, A.qdesc, A.qact, A.qflag, A.slots, nullptr, o_status, o_out, o_flag, res_end,
                          p->nnratio, 0, 0, nullptr, nullptr, nullptr, nullptr, d_ids, false };
            std::vector<uint8_t> occ_tmp;
            uint8_t* occ = r->occupied;
            if (!occ) { occ_tmp.resize(n); occ = occ_tmp.data(); }
            nmatches = frame_window_dev(c, f, D, occ, r->match);
            if (nmatches < 0) return nmatches;
            if (D.host_accept) { if ((rc = frame_fetch(c, r->mp_id, f->mp_id, (size_t)n * 4))) return rc; }
            else std::memcpy(r->mp_id, h + o_ids, (size_t)n * 4);
            std::memcpy(r->in_view_slot, h + o_slots, (size_t)nv * 4);
            for (int i = 0; i < n; i++) if (r->match[i] >= 0) r->match[i] = r->in_view_slot[r->match[i]];   // query -> slot
        }
        if (n == 0) std::memcpy(r->in_view_slot, h + o_slots, (size_t)nv * 4);
        if (taps) {
            if (r->proj_x) std::memcpy(r->proj_x, h + o_px, (size_t)nv * 4);
            if (r->proj_y) std::memcpy(r->proj_y, h + o_py, (size_t)nv * 4);
            if (r->level) std::memcpy(r->level, h + o_lvl, (size_t)nv * 4);
            if (r->view_cos) std::memcpy(r->view_cos, h + o_vc, (size_t)nv * 4);
        }
        return nmatches;
    });
    if (timed) {
        double* t_ms = c->frame->slp_ms;
        t_ms[0] = ms(t_entry, t_before); t_ms[1] = ms(t_before, t_after); t_ms[2] = ms(t_after, clk::now());
    }
    return ret;
}

int ccm_frame_search_local_points_timing(ccm_ctx* c, double out[3])
{
    if (!c || !out) return CCM_E_ARG;
    if (!c->frame || c->frame->slp_ms[0] < 0) return ccm_fail(c, CCM_E_STATE, "no ccm_frame_search_local_points on this context yet");
    std::memcpy(out, c->frame->slp_ms, sizeof c->frame->slp_ms);
    return CCM_OK;
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
    return ccm_guard(c, "ccm_frame_pose_optimize_table", [&]() -> int {
        bool bad_id = false;
        if ((rc = frame_pose_run(c, f, t->T.capacity, nullptr, t->T.pos, t->T.flags, inv_level_sigma2, n_levels, intr, pose7, outlier, n_inliers, &bad_id)))
            return rc;
        if (bad_id) return ccm_fail(c, CCM_E_ARG, "a map-point id outside the table or of a slot that is not LIVE, or an octave outside [0, %d)", n_levels);
        return CCM_OK;
    });
}

// Tracking::TrackWithMotionModel behind the pose product, src/Tracking.cpp:579-621.  Staging, results first:
//   [ status | match | occupied | last_outlier | head | pose7 | intr | inv_sigma2 | scale | n_inliers | outlier | mp_id | u | v | valid ]
// One upload takes last_outlier .. scale (head as zeros); every pass downloads status .. head, the end of the call head .. mp_id, or
// .. valid for the taps.  The queries' radius, level window, HAS_OBS flags and descriptors stay in device memory (FrameState::tmm);
// the id a matched feature receives is read from last's own mp_id (a query's slot is its feature's id), so no id list is made.
int ccm_frame_track_motion_model(ccm_ctx* c, ccm_frame* cur, const ccm_frame* last, ccm_map_table* t, const ccm_tmm_params* p, ccm_tmm_result* r)
{
    RoctxRange roctx_("ccm_frame_track_motion_model");
    if (!c || !cur || !last || !t || !p || !r) return CCM_E_ARG;
    const char* fn = "ccm_frame_track_motion_model";
    int rc;
    if ((rc = frame_named_check(c, cur, fn, "cur")) || (rc = frame_named_check(c, last, fn, "last")) || (rc = check_table(c, t))) return rc;
    const bool pose = p->inv_level_sigma2 != nullptr, taps = r->u != nullptr;
    if (cur == last) return ccm_fail(c, CCM_E_ARG, "%s: cur and last are the same handle", fn);
    if (p->n_levels < 1 || p->n_levels > CCM_MAX_LEVELS) return ccm_fail(c, CCM_E_ARG, "%s: n_levels = %d outside 1..%d", fn, p->n_levels, CCM_MAX_LEVELS);
    if (!p->scale_factors || (pose && !p->intr) || (cur->n > 0 && (!r->match || !r->mp_id || !r->outlier)))
        return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !p->scale_factors ? "scale_factors" : pose && !p->intr ? "intr with inv_level_sigma2" :
                        !r->match ? "match" : !r->mp_id ? "mp_id" : "outlier");
    if ((r->u || r->v || r->valid) && !(r->u && r->v && r->valid)) return ccm_fail(c, CCM_E_ARG, "%s: the taps u, v and valid come together", fn);
    if (p->check_ori && (!cur->has_angle || !last->has_angle)) return ccm_fail(c, CCM_E_ARG, "%s: orientation check against a frame created without angles", fn);
    if (last->n_levels > p->n_levels || (pose && cur->n_levels > p->n_levels))
        return ccm_fail(c, CCM_E_ARG, "%s: octaves up to %d in %s, n_levels = %d", fn, (last->n_levels > p->n_levels ? last : cur)->n_levels - 1,
                        last->n_levels > p->n_levels ? "last" : "cur", p->n_levels);
    return ccm_guard(c, fn, [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        FrameState& S = *frame_state(c);
        hipStream_t st = c->stream;
        const int n = cur->n, nl = last->n;
        r->n_matches = 0; r->passes = 0; r->posed = 0; r->n_inliers = 0; r->n_matches_map = 0;
        if (n == 0 || nl == 0) {                                               // :579 still happens; no matcher, no pose
            if (n > 0) {
                CCM_HIP(c, hipMemsetAsync(cur->mp_id, 0xFF, (size_t)n * 4, st));
                for (int i = 0; i < n; i++) { r->match[i] = -1; r->mp_id[i] = -1; }
                std::memset(r->outlier, 0, n);
            }
            return CCM_OK;
        }
        const size_t m = (size_t)nl;
        size_t off = 0;
        const size_t o_status = seg(off, 16), o_out = seg(off, (size_t)n * 4), o_flag = seg(off, (size_t)n);
        const size_t o_lout = seg(off, p->last_outlier ? m : 0);
        const size_t o_head = seg(off, 16), pass_end = o_head + 16;
        const size_t o_pose = seg(off, 56), o_intr = seg(off, 32), o_is2 = seg(off, CCM_MAX_LEVELS * 4), o_scale = seg(off, CCM_MAX_LEVELS * 4);
        const size_t up_end = off;
        const size_t o_ninl = seg(off, 16), o_outl = seg(off, (size_t)n), o_ids = seg(off, (size_t)n * 4);
        const size_t res_end = o_ids + (size_t)n * 4;
        const size_t o_u = seg(off, m * 4), o_v = seg(off, m * 4), o_act = seg(off, m);
        const size_t tap_end = o_act + m;
        uint8_t* h = nullptr;
        if ((rc = frame_staging(c, off, &h))) return rc;
        size_t w = 0;                                                          // device-only work area
        const size_t w_qr = seg(w, m * 4), w_minl = seg(w, m * 4), w_maxl = seg(w, m * 4), w_qflag = seg(w, m), w_qdesc = seg(w, m * 32);
        CCM_RESERVE(c, S.tmm, w + 64);
        uint8_t* io = S.io.as<uint8_t>(); uint8_t* wk = S.tmm.as<uint8_t>();

        if (p->last_outlier) std::memcpy(h + o_lout, p->last_outlier, m);
        std::memset(h + o_head, 0, up_end - o_head);
        if (pose) { std::memcpy(h + o_pose, r->pose7, 56); std::memcpy(h + o_intr, p->intr, 32); std::memcpy(h + o_is2, p->inv_level_sigma2, (size_t)p->n_levels * 4); }
        std::memcpy(h + o_scale, p->scale_factors, (size_t)p->n_levels * 4);
        if ((rc = frame_upload(c, o_lout, up_end))) return rc;                 // 5 segments of 64 bytes, and last_outlier when given

        int* d_head = (int*)(io + o_head); int* d_out = (int*)(io + o_out); uint8_t* d_flag = io + o_flag;
        TmmArgs A{};
        A.n_last = nl; A.last_id = last->mp_id; A.last_outlier = p->last_outlier ? io + o_lout : nullptr;
        std::memcpy(A.Tcw, p->Tcw, sizeof A.Tcw);
        A.fx = p->fx; A.fy = p->fy; A.cx = p->cx; A.cy = p->cy; A.min_x = p->min_x; A.max_x = p->max_x; A.min_y = p->min_y; A.max_y = p->max_y;
        A.qx = (float*)(io + o_u); A.qy = (float*)(io + o_v); A.act = io + o_act; A.qflag = wk + w_qflag; A.qdesc = wk + w_qdesc; A.head = d_head;
        tmm_launch_project(st, A, t->T);
        CCM_HIP(c, hipGetLastError());

        std::vector<uint8_t> occ(n);
        int nm = 0, passes = 0;
        for (int pass = 0; pass < 2; pass++) {
            const float th = pass == 0 ? p->th : 2.0f * p->th;
            tmm_launch_clear(st, n, nl, d_head, cur->mp_id, d_out, d_flag, A.act);
            frame_launch_prep_last(st, nl, A.act, last->oct, (const float*)(io + o_scale), th, (float*)(wk + w_qr), (int*)(wk + w_minl), (int*)(wk + w_maxl));
            CCM_HIP(c, hipGetLastError());
            WinDevCall D{ 2, nl, A.qx, A.qy, (const float*)(wk + w_qr), (const int*)(wk + w_minl), (const int*)(wk + w_maxl), A.qdesc, A.act, A.qflag,
                          last->mp_id, last->angle, o_status, o_out, o_flag, pass_end, 0.f, p->orb_dist, p->check_ori ? 1 : 0,
                          nullptr, nullptr, nullptr, last, nullptr, false };
            nm = frame_window_dev(c, cur, D, occ.data(), r->match);
            if (nm < 0) return nm;
            passes = pass + 1;
            if (pass == 0) {                                                   // the projection's verdict came back with the first pass
                int bad = 0;
                if (D.host_accept) { if ((rc = frame_fetch(c, &bad, d_head, 4))) return rc; }
                else std::memcpy(&bad, h + o_head, 4);
                if (bad) return ccm_fail(c, CCM_E_ARG, "%s: last holds a map-point id outside [0, %d) or of a slot that is not LIVE", fn, t->capacity);
            }
            if (!(nm < p->retry_below)) break;
        }
        r->n_matches = nm; r->passes = passes;

        const bool posed = pose && nm >= p->min_matches;
        if (posed && (rc = frame_pose_queue(c, cur, t->T.capacity, t->T.pos, t->T.flags, p->n_levels, PoseIo{ o_ninl, o_outl, o_pose, o_intr, o_is2, 0 })))
            return rc;
        tmm_launch_discard(st, n, cur->mp_id, posed ? io + o_outl : nullptr, t->T, (int*)(io + o_ids), d_head);
        CCM_HIP(c, hipGetLastError());
        if ((rc = frame_fetch(c, h + o_head, io + o_head, (taps ? tap_end : res_end) - o_head))) return rc;
        int head[2], ninl[2] = { 0, 0 };
        std::memcpy(head, h + o_head, 8);
        if (posed) {
            std::memcpy(ninl, h + o_ninl, 8);
            if (ninl[1]) return ccm_fail(c, CCM_E_DEVICE, "%s: the pose stage met an id or octave it cannot use", fn);   // checked on entry and by the projection
            std::memcpy(r->pose7, h + o_pose, 56);
            std::memcpy(r->outlier, h + o_outl, n);
        } else std::memset(r->outlier, 0, n);
        std::memcpy(r->mp_id, h + o_ids, (size_t)n * 4);
        r->posed = posed ? 1 : 0; r->n_inliers = ninl[0]; r->n_matches_map = head[1];
        if (taps) { std::memcpy(r->u, h + o_u, m * 4); std::memcpy(r->v, h + o_v, m * 4); std::memcpy(r->valid, h + o_act, m); }
        return CCM_OK;
    });
}

}  // extern "C"
