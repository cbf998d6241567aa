// map_host.cpp -- C ABI of LocalMapping::CreateNewMapPoints (src/Mapping.cpp:284-469).  ccm_create_new_map_points checks the
// arguments, applies the baseline rule (:319-328), orders every neighbour's candidate features by vocabulary node with a counting
// pass, flattens everything into one page-locked staging area (one upload), queues the three launches of map_kernels.hip and one
// download of the result list, and synchronises once.  The tap arrays are downloaded only when a tap is given.
// ccm_create_new_map_points_frames is the same call on frame handles (frame_internal.h): the keyframes already lie in device memory
// in node order, so the staged upload holds the per-neighbour MapKf records and a table of per-keyframe device views, nothing else.
#include "frame_internal.h"
#include "map_types.h"
#include <cmath>

// One page-locked staging area and its device twin, laid out [inputs | per-pair work arrays | result list], and the node table of the
// counting pass: cid[node] = 1 + compact id of a node of the current keyframe, all zero between calls.
struct MapState { DevBuf io; uint8_t* host = nullptr; size_t host_cap = 0; std::vector<int32_t> cid; };
void map_state_free(MapState* s)
{
    if (!s) return;
    if (s->host) (void)hipHostFree(s->host);
    delete s;
}

// map_math.h names the statuses itself (it is compiled without the ABI header too)
static_assert((int)MAP_SKIPPED_KF == (int)CCM_NP_SKIPPED_KF && (int)MAP_NO_MATCH == (int)CCM_NP_NO_MATCH && (int)MAP_NONFINITE == (int)CCM_NP_NONFINITE &&
              (int)MAP_BEHIND_1 == (int)CCM_NP_BEHIND_1 && (int)MAP_SCALE == (int)CCM_NP_SCALE && (int)MAP_OK == (int)CCM_NP_OK &&
              (int)MAP_SUPERSEDED == (int)CCM_NP_SUPERSEDED,
              "MAP_* of map_math.h and CCM_NP_* of ccm_hot.h are one list");

static const int kMaxNode = 1 << 24, kMaxFeatures = (1 << MAP_POS_BITS) - 1;

// Argument check of one keyframe; `who` names it in the message.
static int check_keyframe(ccm_ctx* c, const ccm_map_keyframe* kf, const char* who, int min_levels)
{
    const char* fn = "ccm_create_new_map_points";
    if (kf->n < 0 || kf->n > kMaxFeatures) return ccm_fail(c, CCM_E_ARG, "%s: %s.n = %d outside [0, %d]", fn, who, kf->n, kMaxFeatures);
    if (!kf->Tcw || !kf->Ow) return ccm_fail(c, CCM_E_ARG, "%s: null %s.%s", fn, who, !kf->Tcw ? "Tcw" : "Ow");
    if (!kf->scale_factors || !kf->level_sigma2) return ccm_fail(c, CCM_E_ARG, "%s: null %s.%s", fn, who, !kf->scale_factors ? "scale_factors" : "level_sigma2");
    if (kf->n_levels < min_levels) return ccm_fail(c, CCM_E_ARG, "%s: %s.n_levels = %d, at least %d needed", fn, who, kf->n_levels, min_levels);
    if (kf->n == 0) return CCM_OK;
    const void* arr[] = { kf->kp_x, kf->kp_y, kf->kp_octave, kf->desc, kf->node, kf->has_mp };
    const char* name[] = { "kp_x", "kp_y", "kp_octave", "desc", "node", "has_mp" };
    for (int a = 0; a < 6; a++) if (!arr[a]) return ccm_fail(c, CCM_E_ARG, "%s: null %s.%s", fn, who, name[a]);
    for (int i = 0; i < kf->n; i++) {
        if (kf->kp_octave[i] < 0 || kf->kp_octave[i] >= kf->n_levels)
            return ccm_fail(c, CCM_E_ARG, "%s: %s.kp_octave[%d] = %d outside [0, %d)", fn, who, i, kf->kp_octave[i], kf->n_levels);
        if (kf->node[i] >= kMaxNode) return ccm_fail(c, CCM_E_ARG, "%s: %s.node[%d] = %d, not below %d", fn, who, i, kf->node[i], kMaxNode);
    }
    return CCM_OK;
}

static void fill_cam(const ccm_map_keyframe& kf, MapCam& m)
{
    m.fx = kf.fx; m.fy = kf.fy; m.cx = kf.cx; m.cy = kf.cy;
    m.invfx = 1.0f / kf.fx; m.invfy = 1.0f / kf.fy;                        // KeyFrame::invfx, invfy
    std::memcpy(m.Tcw, kf.Tcw, 48); std::memcpy(m.Ow, kf.Ow, 12);
    m.pad_[0] = m.pad_[1] = m.pad_[2] = 0.0f;
}
static inline MapFeat feat_of(const ccm_map_keyframe& kf, int i)
{
    const int o = kf.kp_octave[i];
    return MapFeat{ kf.kp_x[i], kf.kp_y[i], kf.level_sigma2[o], kf.scale_factors[o] };
}

extern "C" int ccm_create_new_map_points(ccm_ctx* c, const ccm_new_points_problem* pb, ccm_new_points_result* res)
{
    RoctxRange roctx_("ccm_create_new_map_points");
    return ccm_guard(c, "ccm_create_new_map_points", [&]() -> int {
        const char* fn = "ccm_create_new_map_points";
        if (!pb || !res) return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !pb ? "problem" : "result");
        if (!pb->current) return ccm_fail(c, CCM_E_ARG, "%s: null current", fn);
        if (pb->n_kf < 0) return ccm_fail(c, CCM_E_ARG, "%s: n_kf = %d", fn, pb->n_kf);
        const int n_kf = pb->n_kf;
        if (n_kf > 0 && (!pb->neighbours || !pb->F12 || !pb->epipole || !pb->median_depth))
            return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !pb->neighbours ? "neighbours" : !pb->F12 ? "F12" : !pb->epipole ? "epipole" : "median_depth");
        const ccm_map_keyframe& cur = *pb->current;
        int rc = check_keyframe(c, &cur, "current", 2);                      // ratioFactor reads scale_factors[1]
        if (rc) return rc;
        const int n1 = cur.n;
        for (int k = 0; k < n_kf; k++) {
            char who[40];
            snprintf(who, sizeof who, "neighbours[%d]", k);
            if ((rc = check_keyframe(c, &pb->neighbours[k], who, 1))) return rc;
            if (!(pb->median_depth[k] > 0.0f)) return ccm_fail(c, CCM_E_ARG, "%s: median_depth[%d] = %g is not positive", fn, k, (double)pb->median_depth[k]);
        }
        if (!res->first) return ccm_fail(c, CCM_E_ARG, "%s: null first", fn);
        if (n1 > 0 && (!res->kf || !res->idx1 || !res->idx2 || !res->x3d))
            return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !res->kf ? "kf" : !res->idx1 ? "idx1" : !res->idx2 ? "idx2" : "x3d");
        if ((long long)n_kf * n1 > (1ll << 30)) return ccm_fail(c, CCM_E_ARG, "%s: n_kf * current.n = %lld above 2^30", fn, (long long)n_kf * n1);
        ccm_new_points_tap* tap = res->tap;
        if (n_kf == 0 || n1 == 0) {                                          // nothing to match: no device work
            for (int k = 0; k <= n_kf; k++) res->first[k] = 0;
            res->n_new = 0;
            return 0;
        }
        if (!c) return CCM_E_ARG;                                            // everything above needs no context
        CCM_HIP(c, hipSetDevice(c->device));
        if (!c->map) c->map = new MapState();
        MapState& St = *c->map;

        // ---- the current keyframe's nodes, compacted in order of first appearance; the table is cleared again when the call leaves
        int max_node = -1;
        for (int i = 0; i < n1; i++) if (!cur.has_mp[i]) max_node = std::max(max_node, cur.node[i]);
        if ((size_t)(max_node + 1) > St.cid.size()) St.cid.resize((size_t)max_node + 1, 0);
        struct Clear {
            std::vector<int32_t>& cid; const ccm_map_keyframe& kf;
            ~Clear() { for (int i = 0; i < kf.n; i++) if (!kf.has_mp[i] && kf.node[i] >= 0) cid[kf.node[i]] = 0; }
        } clear_{ St.cid, cur };
        const std::vector<int32_t>& cid = St.cid;
        std::vector<int32_t> cnode1(n1), free1;
        int n_nodes = 0;
        for (int i = 0; i < n1; i++) {
            if (cur.has_mp[i]) { cnode1[i] = -2; continue; }                 // :744-746
            const int nd = cur.node[i];
            if (nd < 0) { cnode1[i] = -1; continue; }
            if (!St.cid[nd]) St.cid[nd] = ++n_nodes;
            cnode1[i] = St.cid[nd] - 1;
            free1.push_back(i);
        }
        const int n_free = (int)free1.size();
        // compact node of a neighbour's feature that can be a candidate, or -1 (:763: no map point; a node the current keyframe has)
        auto cand_node = [&](const ccm_map_keyframe& kf, int i) -> int {
            const int nd = kf.node[i];
            return (kf.has_mp[i] || nd < 0 || (size_t)nd >= cid.size()) ? -1 : cid[nd] - 1;
        };
        // ---- counting pass: range[k][node] = (first position, length) in the flattened side 2
        std::vector<int32_t> range(2 * (size_t)n_kf * std::max(n_nodes, 1), 0);
        long long m2 = 0;
        for (int k = 0; k < n_kf && n_nodes > 0; k++) {
            const ccm_map_keyframe& kf = pb->neighbours[k];
            int32_t* rg = range.data() + 2 * (size_t)k * n_nodes;
            for (int i = 0; i < kf.n; i++) { const int cn = cand_node(kf, i); if (cn >= 0) rg[2 * cn + 1]++; }
            for (int cn = 0; cn < n_nodes; cn++) { rg[2 * cn] = (int32_t)m2; m2 += rg[2 * cn + 1]; }
            if (m2 > 0x7fffffffll) return ccm_fail(c, CCM_E_ARG, "%s: more than 2^31 candidate features", fn);
        }

        // ---- staging
        const size_t pairs = (size_t)n_kf * n1;
        size_t off = 0;
        const size_t o_cam = seg(off, (size_t)(1 + n_kf) * sizeof(MapCam)), o_kf = seg(off, (size_t)n_kf * sizeof(MapKf));
        const size_t o_f1 = seg(off, (size_t)n1 * sizeof(MapFeat)), o_d1 = seg(off, (size_t)n1 * 32), o_cn = seg(off, (size_t)n1 * 4);
        const size_t o_free = seg(off, (size_t)n_free * 4), o_rg = seg(off, range.size() * 4);
        const size_t o_f2 = seg(off, (size_t)m2 * sizeof(MapFeat)), o_d2 = seg(off, (size_t)m2 * 32), o_i2 = seg(off, (size_t)m2 * 4);
        const size_t in_end = off;
        const size_t o_mpos = seg(off, pairs * 4), o_gate = seg(off, pairs), o_status = seg(off, pairs), o_X = seg(off, pairs * 12);
        const size_t work_end = off;
        const size_t o_first = seg(off, (size_t)(n_kf + 1) * 4), o_okf = seg(off, (size_t)n1 * 4), o_oi1 = seg(off, (size_t)n1 * 4);
        const size_t o_oi2 = seg(off, (size_t)n1 * 4), o_ox = seg(off, (size_t)n1 * 12);
        const size_t end = off;
        if (end > St.host_cap) {
            if (St.host) (void)hipHostFree(St.host);
            St.host = nullptr; St.host_cap = 0;
            const size_t want = end + end / 4 + 4096;
            if (hipHostMalloc((void**)&St.host, want, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError(); St.host = nullptr;
                return ccm_fail(c, CCM_E_NOMEM, "page-locked staging of %zu bytes failed", want);
            }
            St.host_cap = want;
        }
        CCM_RESERVE(c, St.io, end);
        uint8_t* h = St.host;                                                // free: every call ends with a synchronisation
        MapCam* cam = reinterpret_cast<MapCam*>(h + o_cam);
        MapKf* hkf = reinterpret_cast<MapKf*>(h + o_kf);
        fill_cam(cur, cam[0]);
        for (int k = 0; k < n_kf; k++) {
            const ccm_map_keyframe& kf = pb->neighbours[k];
            fill_cam(kf, cam[1 + k]);
            hkf[k].skipped = map_baseline_too_short(cur.Ow, kf.Ow, pb->median_depth[k]) ? 1 : 0;
            hkf[k].ex = pb->epipole[2 * k]; hkf[k].ey = pb->epipole[2 * k + 1];
            std::memcpy(hkf[k].F12, pb->F12 + 9 * (size_t)k, 36);
        }
        MapFeat* hf1 = reinterpret_cast<MapFeat*>(h + o_f1);
        for (int i = 0; i < n1; i++) hf1[i] = feat_of(cur, i);
        std::memcpy(h + o_d1, cur.desc, (size_t)n1 * 32);
        std::memcpy(h + o_cn, cnode1.data(), (size_t)n1 * 4);
        if (n_free) std::memcpy(h + o_free, free1.data(), (size_t)n_free * 4);
        std::memcpy(h + o_rg, range.data(), range.size() * 4);
        MapFeat* hf2 = reinterpret_cast<MapFeat*>(h + o_f2);
        uint8_t* hd2 = h + o_d2;
        int32_t* hi2 = reinterpret_cast<int32_t*>(h + o_i2);
        std::vector<int32_t> fill(std::max(n_nodes, 1));
        for (int k = 0; k < n_kf && n_nodes > 0; k++) {                      // ascending index inside a node: the order DBoW2 fills a FeatureVector in
            const ccm_map_keyframe& kf = pb->neighbours[k];
            const int32_t* rg = range.data() + 2 * (size_t)k * n_nodes;
            for (int cn = 0; cn < n_nodes; cn++) fill[cn] = rg[2 * cn];
            for (int i = 0; i < kf.n; i++) {
                const int cn = cand_node(kf, i);
                if (cn < 0) continue;
                const size_t p = (size_t)fill[cn]++;
                hf2[p] = feat_of(kf, i);
                std::memcpy(hd2 + 32 * p, kf.desc + 32 * (size_t)i, 32);
                hi2[p] = i;
            }
        }
        hipStream_t st = c->stream;
        uint8_t* d = St.io.as<uint8_t>();
        CCM_HIP(c, hipMemcpyAsync(d, h, in_end, hipMemcpyHostToDevice, st));
        MapDev D{};
        D.n1 = n1; D.n_kf = n_kf; D.n_free = n_free; D.n_nodes = n_nodes;
        D.ratioFactor = 1.5f * cur.scale_factors[1];                         // :307
        D.cam = reinterpret_cast<const MapCam*>(d + o_cam); D.kf = reinterpret_cast<const MapKf*>(d + o_kf);
        D.f1 = reinterpret_cast<const MapFeat*>(d + o_f1); D.desc1 = d + o_d1; D.cnode1 = reinterpret_cast<const int32_t*>(d + o_cn);
        D.free1 = reinterpret_cast<const int32_t*>(d + o_free); D.range = reinterpret_cast<const int32_t*>(d + o_rg);
        D.f2 = reinterpret_cast<const MapFeat*>(d + o_f2); D.desc2 = d + o_d2; D.idx2 = reinterpret_cast<const int32_t*>(d + o_i2);
        D.mpos = reinterpret_cast<int32_t*>(d + o_mpos); D.gate = d + o_gate; D.status = d + o_status; D.X = reinterpret_cast<float*>(d + o_X);
        D.first = reinterpret_cast<int32_t*>(d + o_first); D.out_kf = reinterpret_cast<int32_t*>(d + o_okf);
        D.out_idx1 = reinterpret_cast<int32_t*>(d + o_oi1); D.out_idx2 = reinterpret_cast<int32_t*>(d + o_oi2); D.out_x3d = reinterpret_cast<float*>(d + o_ox);
        map_match_launch(st, D);
        map_triangulate_launch(st, D);
        map_resolve_launch(st, D);
        CCM_HIP(c, hipGetLastError());
        CCM_HIP(c, hipMemcpyAsync(h + work_end, d + work_end, end - work_end, hipMemcpyDeviceToHost, st));
        const bool want_tap = tap && (tap->match || tap->status || tap->x3d_all);
        if (want_tap) CCM_HIP(c, hipMemcpyAsync(h + in_end, d + in_end, work_end - in_end, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipStreamSynchronize(st));

        // ---- outputs
        const int32_t* first = reinterpret_cast<const int32_t*>(h + o_first);
        const int n_new = first[n_kf];
        if (n_new < 0 || n_new > n1) return ccm_fail(c, CCM_E_DEVICE, "%s: the device reported %d new points for %d features", fn, n_new, n1);
        std::memcpy(res->first, first, (size_t)(n_kf + 1) * 4);
        std::memcpy(res->kf, h + o_okf, (size_t)n_new * 4); std::memcpy(res->idx1, h + o_oi1, (size_t)n_new * 4);
        std::memcpy(res->idx2, h + o_oi2, (size_t)n_new * 4); std::memcpy(res->x3d, h + o_ox, (size_t)n_new * 12);
        res->n_new = n_new;
        if (want_tap) {
            if (tap->match) {
                const int32_t* mpos = reinterpret_cast<const int32_t*>(h + o_mpos);
                for (int k = 0; k < n_kf; k++)
                    for (int i = 0; i < n1; i++) {
                        const size_t t = (size_t)k * n1 + i;
                        tap->match[t] = (cnode1[i] >= 0 && mpos[t] >= 0) ? hi2[mpos[t]] : -1;      // mpos is written for the features of free1 only
                    }
            }
            if (tap->status) std::memcpy(tap->status, h + o_status, pairs);
            if (tap->x3d_all) std::memcpy(tap->x3d_all, h + o_X, pairs * 12);
        }
        return n_new;
    });
}

static MapKfView view_of(const ccm_frame* f)
{
    return MapKfView{ f->d_cam, f->kx, f->ky, f->oct, f->mp_id, f->desc, f->sf, f->sig2, f->node, f->order, f->nodes, f->first, f->feat_o, f->desc_o,
                      f->n, f->n_nodes };
}

extern "C" int ccm_create_new_map_points_frames(ccm_ctx* c, const ccm_new_points_frames* pb, ccm_new_points_result* res)
{
    RoctxRange roctx_("ccm_create_new_map_points_frames");
    return ccm_guard(c, "ccm_create_new_map_points_frames", [&]() -> int {
        const char* fn = "ccm_create_new_map_points_frames";
        if (!c) return CCM_E_ARG;
        if (!pb || !res) return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !pb ? "problem" : "result");
        if (!pb->current) return ccm_fail(c, CCM_E_ARG, "%s: null current", fn);
        if (pb->n_kf < 0) return ccm_fail(c, CCM_E_ARG, "%s: n_kf = %d", fn, pb->n_kf);
        const int n_kf = pb->n_kf;
        if (n_kf > 0 && (!pb->neighbours || !pb->F12 || !pb->epipole || !pb->median_depth))
            return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !pb->neighbours ? "neighbours" : !pb->F12 ? "F12" : !pb->epipole ? "epipole" : "median_depth");
        const ccm_frame* cur = pb->current;
        auto check_handle = [&](const ccm_frame* f, const char* who) -> int {
            if (!f) return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, who);
            if (!f->ctx || f->ctx != c) return ccm_fail(c, CCM_E_ARG, "%s: %s %s", fn, who, !f->ctx ? "outlived its context" : "belongs to another context");
            return CCM_OK;
        };
        int rc = check_handle(cur, "current");
        if (rc) return rc;
        const int n1 = cur->n;
        char who[40];
        for (int k = 0; k < n_kf; k++) {
            snprintf(who, sizeof who, "neighbours[%d]", k);
            if ((rc = check_handle(pb->neighbours[k], who))) return rc;
            if (!(pb->median_depth[k] > 0.0f)) return ccm_fail(c, CCM_E_ARG, "%s: median_depth[%d] = %g is not positive", fn, k, (double)pb->median_depth[k]);
        }
        if (!res->first) return ccm_fail(c, CCM_E_ARG, "%s: null first", fn);
        if (n1 > 0 && (!res->kf || !res->idx1 || !res->idx2 || !res->x3d))
            return ccm_fail(c, CCM_E_ARG, "%s: null %s", fn, !res->kf ? "kf" : !res->idx1 ? "idx1" : !res->idx2 ? "idx2" : "x3d");
        if ((long long)n_kf * n1 > (1ll << 30)) return ccm_fail(c, CCM_E_ARG, "%s: n_kf * current.n = %lld above 2^30", fn, (long long)n_kf * n1);
        if (n_kf == 0 || n1 == 0) {                                          // nothing to match: no device work
            for (int k = 0; k <= n_kf; k++) res->first[k] = 0;
            res->n_new = 0;
            return 0;
        }
        if (const char* lacks = frame_keyframe_lacks(cur)) return ccm_fail(c, CCM_E_STATE, "%s: current: no %s", fn, lacks);
        for (int k = 0; k < n_kf; k++)
            if (const char* lacks = frame_keyframe_lacks(pb->neighbours[k])) return ccm_fail(c, CCM_E_STATE, "%s: neighbours[%d]: no %s", fn, k, lacks);
        if (cur->cam_levels < 2) return ccm_fail(c, CCM_E_ARG, "%s: current.n_levels = %d, at least 2 needed", fn, cur->cam_levels);   // ratioFactor reads scale_factors[1]
        ccm_new_points_tap* tap = res->tap;
        CCM_HIP(c, hipSetDevice(c->device));
        if (!c->map) c->map = new MapState();
        MapState& St = *c->map;

        // ---- staging: [MapKf | views] up, [per-pair work arrays] and [result list] down
        const size_t pairs = (size_t)n_kf * n1;
        size_t off = 0;
        const size_t o_kf = seg(off, (size_t)n_kf * sizeof(MapKf)), o_view = seg(off, (size_t)(1 + n_kf) * sizeof(MapKfView));
        const size_t in_end = off;
        const size_t o_midx = seg(off, pairs * 4), o_gate = seg(off, pairs), o_status = seg(off, pairs), o_X = seg(off, pairs * 12);
        const size_t work_end = off;
        const size_t o_first = seg(off, (size_t)(n_kf + 1) * 4), o_okf = seg(off, (size_t)n1 * 4), o_oi1 = seg(off, (size_t)n1 * 4);
        const size_t o_oi2 = seg(off, (size_t)n1 * 4), o_ox = seg(off, (size_t)n1 * 12);
        const size_t end = off;
        if (end > St.host_cap) {
            if (St.host) (void)hipHostFree(St.host);
            St.host = nullptr; St.host_cap = 0;
            const size_t want = end + end / 4 + 4096;
            if (hipHostMalloc((void**)&St.host, want, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError(); St.host = nullptr;
                return ccm_fail(c, CCM_E_NOMEM, "page-locked staging of %zu bytes failed", want);
            }
            St.host_cap = want;
        }
        CCM_RESERVE(c, St.io, end);
        uint8_t* h = St.host;                                                // free: every call ends with a synchronisation
        MapKf* hkf = reinterpret_cast<MapKf*>(h + o_kf);
        MapKfView* hv = reinterpret_cast<MapKfView*>(h + o_view);
        hv[0] = view_of(cur);
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* kf = pb->neighbours[k];
            hv[1 + k] = view_of(kf);
            hkf[k].skipped = map_baseline_too_short(cur->cam.Ow, kf->cam.Ow, pb->median_depth[k]) ? 1 : 0;   // :319-328 on the handles' host copies
            hkf[k].ex = pb->epipole[2 * k]; hkf[k].ey = pb->epipole[2 * k + 1];
            std::memcpy(hkf[k].F12, pb->F12 + 9 * (size_t)k, 36);
        }
        hipStream_t st = c->stream;
        uint8_t* d = St.io.as<uint8_t>();
        CCM_HIP(c, hipMemcpyAsync(d, h, in_end, hipMemcpyHostToDevice, st));
        MapFramesDev D{};
        D.n1 = n1; D.n_kf = n_kf;
        D.ratioFactor = 1.5f * cur->sf1;                                     // :307
        D.kf = reinterpret_cast<const MapKf*>(d + o_kf); D.view = reinterpret_cast<const MapKfView*>(d + o_view);
        D.midx = reinterpret_cast<int32_t*>(d + o_midx); D.gate = d + o_gate; D.status = d + o_status; D.X = reinterpret_cast<float*>(d + o_X);
        D.first = reinterpret_cast<int32_t*>(d + o_first); D.out_kf = reinterpret_cast<int32_t*>(d + o_okf);
        D.out_idx1 = reinterpret_cast<int32_t*>(d + o_oi1); D.out_idx2 = reinterpret_cast<int32_t*>(d + o_oi2); D.out_x3d = reinterpret_cast<float*>(d + o_ox);
        map_frames_launch(st, D);
        CCM_HIP(c, hipGetLastError());
        CCM_HIP(c, hipMemcpyAsync(h + work_end, d + work_end, end - work_end, hipMemcpyDeviceToHost, st));
        const bool want_tap = tap && (tap->match || tap->status || tap->x3d_all);
        if (want_tap) CCM_HIP(c, hipMemcpyAsync(h + in_end, d + in_end, work_end - in_end, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipStreamSynchronize(st));

        // ---- outputs
        const int32_t* first = reinterpret_cast<const int32_t*>(h + o_first);
        const int n_new = first[n_kf];
        if (n_new < 0 || n_new > n1) return ccm_fail(c, CCM_E_DEVICE, "%s: the device reported %d new points for %d features", fn, n_new, n1);
        std::memcpy(res->first, first, (size_t)(n_kf + 1) * 4);
        std::memcpy(res->kf, h + o_okf, (size_t)n_new * 4); std::memcpy(res->idx1, h + o_oi1, (size_t)n_new * 4);
        std::memcpy(res->idx2, h + o_oi2, (size_t)n_new * 4); std::memcpy(res->x3d, h + o_ox, (size_t)n_new * 12);
        res->n_new = n_new;
        if (want_tap) {
            if (tap->match) std::memcpy(tap->match, h + o_midx, pairs * 4);
            if (tap->status) std::memcpy(tap->status, h + o_status, pairs);
            if (tap->x3d_all) std::memcpy(tap->x3d_all, h + o_X, pairs * 12);
        }
        return n_new;
    });
}
