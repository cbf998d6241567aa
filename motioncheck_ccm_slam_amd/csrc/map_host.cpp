// map_host.cpp -- C ABI of LocalMapping::CreateNewMapPoints (src/Mapping.cpp:284-469).  ccm_create_new_map_points checks the
// arguments, applies the baseline rule (:319-328), orders every neighbour's candidate features by vocabulary node with a counting
// pass, flattens everything into one page-locked staging area (one upload), queues the three launches of map_kernels.hip and one
// download of the result list, and synchronises once.  The tap arrays are downloaded only when a tap is given.
// ccm_create_new_map_points_frames is the same call on frame handles (frame_internal.h): the keyframes already lie in device memory
// in node order, so the staged upload holds the per-neighbour MapKf records and a table of per-keyframe device views, nothing else.
// ccm_map_pair_geometry and ccm_scene_median_depth define, on the host, the three per-neighbour inputs of both calls (map_math.h).
#include "frame_internal.h"
#include "map_types.h"
#include <cmath>

// The staging area (staging.h), laid out [inputs | per-pair work arrays | result list], and the node table of the counting pass:
// cid[node] = 1 + compact id of a node of the current keyframe, all zero between calls.
struct MapState { Staging stage{ false }; std::vector<int32_t> cid; };
void map_state_free(MapState* s)
{
    if (!s) return;
    s->stage.release();
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

// What both entry points stage behind their inputs: the per-pair work arrays (downloaded for a tap only) and the result list.
struct MapOut { size_t in_end, match, gate, status, X, work_end, first, okf, oi1, oi2, ox, end; };
static MapOut map_out_layout(size_t off, int n_kf, int n1)
{
    const size_t pairs = (size_t)n_kf * n1;
    MapOut o;
    o.in_end = off;
    o.match = seg(off, pairs * 4); o.gate = seg(off, pairs); o.status = seg(off, pairs); o.X = seg(off, pairs * 12);
    o.work_end = off;
    o.first = seg(off, (size_t)(n_kf + 1) * 4); o.okf = seg(off, (size_t)n1 * 4); o.oi1 = seg(off, (size_t)n1 * 4);
    o.oi2 = seg(off, (size_t)n1 * 4); o.ox = seg(off, (size_t)n1 * 12);
    o.end = off;
    return o;
}

// The end of both entry points, behind their launches: the result list comes down, and the work arrays with it when a tap is given;
// one synchronisation; the outputs.  The match tap of the flattened call holds positions in its side 2 (written for the features
// with a compact node only), translated through idx2 [positions]; the handles' call (idx2 == nullptr) holds feature indices already.
static int map_finish(ccm_ctx* c, Staging& G, const char* fn, const MapOut& o, int n_kf, int n1, const int32_t* cnode1, const int32_t* idx2,
                      ccm_new_points_result* res)
{
    const size_t pairs = (size_t)n_kf * n1;
    ccm_new_points_tap* tap = res->tap;
    const bool want_tap = tap && (tap->match || tap->status || tap->x3d_all);
    int rc;
    if ((rc = G.download(c, o.work_end, o.end)) || (want_tap && (rc = G.download(c, o.in_end, o.work_end))) || (rc = G.wait(c))) return rc;
    const int32_t* first = G.host<int32_t>(o.first);
    const int n_new = first[n_kf];
    if (n_new < 0 || n_new > n1) return ccm_fail(c, CCM_E_DEVICE, "%s: the device reported %d new points for %d features", fn, n_new, n1);
    std::memcpy(res->first, first, (size_t)(n_kf + 1) * 4);
    G.get(res->kf, o.okf, (size_t)n_new * 4); G.get(res->idx1, o.oi1, (size_t)n_new * 4);
    G.get(res->idx2, o.oi2, (size_t)n_new * 4); G.get(res->x3d, o.ox, (size_t)n_new * 12);
    res->n_new = n_new;
    if (want_tap) {
        if (tap->match && idx2) {
            const int32_t* mpos = G.host<int32_t>(o.match);
            for (int k = 0; k < n_kf; k++)
                for (int i = 0; i < n1; i++) {
                    const size_t t = (size_t)k * n1 + i;
                    tap->match[t] = (cnode1[i] >= 0 && mpos[t] >= 0) ? idx2[mpos[t]] : -1;
                }
        } else G.get(tap->match, o.match, pairs * 4);
        G.get(tap->status, o.status, pairs); G.get(tap->x3d_all, o.X, pairs * 12);
    }
    return n_new;
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
        if (n_kf == 0 || n1 == 0) {                                          // nothing to match: no device work
            for (int k = 0; k <= n_kf; k++) res->first[k] = 0;
            res->n_new = 0;
            return 0;
        }
        if (!c) return CCM_E_ARG;                                            // everything above needs no context
        CCM_HIP(c, hipSetDevice(c->device));
        if (!c->map) c->map = new MapState();
        MapState& St = *c->map;
        Staging& G = St.stage;

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
        size_t off = 0;
        const size_t o_cam = seg(off, (size_t)(1 + n_kf) * sizeof(MapCam)), o_kf = seg(off, (size_t)n_kf * sizeof(MapKf));
        const size_t o_f1 = seg(off, (size_t)n1 * sizeof(MapFeat)), o_d1 = seg(off, (size_t)n1 * 32), o_cn = seg(off, (size_t)n1 * 4);
        const size_t o_free = seg(off, (size_t)n_free * 4), o_rg = seg(off, range.size() * 4);
        const size_t o_f2 = seg(off, (size_t)m2 * sizeof(MapFeat)), o_d2 = seg(off, (size_t)m2 * 32), o_i2 = seg(off, (size_t)m2 * 4);
        const MapOut o = map_out_layout(off, n_kf, n1);
        if ((rc = G.reserve(c, o.end))) return rc;
        MapCam* cam = G.host<MapCam>(o_cam);
        MapKf* hkf = G.host<MapKf>(o_kf);
        fill_cam(cur, cam[0]);
        for (int k = 0; k < n_kf; k++) {
            const ccm_map_keyframe& kf = pb->neighbours[k];
            fill_cam(kf, cam[1 + k]);
            hkf[k].skipped = map_baseline_too_short(cur.Ow, kf.Ow, pb->median_depth[k]) ? 1 : 0;
            hkf[k].ex = pb->epipole[2 * k]; hkf[k].ey = pb->epipole[2 * k + 1];
            std::memcpy(hkf[k].F12, pb->F12 + 9 * (size_t)k, 36);
        }
        MapFeat* hf1 = G.host<MapFeat>(o_f1);
        for (int i = 0; i < n1; i++) hf1[i] = feat_of(cur, i);
        G.put(o_d1, cur.desc, (size_t)n1 * 32);
        G.put(o_cn, cnode1.data(), (size_t)n1 * 4);
        G.put(o_free, free1.data(), (size_t)n_free * 4);
        G.put(o_rg, range.data(), range.size() * 4);
        MapFeat* hf2 = G.host<MapFeat>(o_f2);
        uint8_t* hd2 = G.host<uint8_t>(o_d2);
        int32_t* hi2 = G.host<int32_t>(o_i2);
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
        if ((rc = G.upload(c, 0, o.in_end))) return rc;
        MapDev D{};
        D.n1 = n1; D.n_kf = n_kf; D.n_free = n_free; D.n_nodes = n_nodes;
        D.ratioFactor = 1.5f * cur.scale_factors[1];                         // :307
        D.cam = G.dev<MapCam>(o_cam); D.kf = G.dev<MapKf>(o_kf);
        D.f1 = G.dev<MapFeat>(o_f1); D.desc1 = G.dev<uint8_t>(o_d1); D.cnode1 = G.dev<int32_t>(o_cn);
        D.free1 = G.dev<int32_t>(o_free); D.range = G.dev<int32_t>(o_rg);
        D.f2 = G.dev<MapFeat>(o_f2); D.desc2 = G.dev<uint8_t>(o_d2); D.idx2 = G.dev<int32_t>(o_i2);
        D.mpos = G.dev<int32_t>(o.match); D.gate = G.dev<uint8_t>(o.gate); D.status = G.dev<uint8_t>(o.status); D.X = G.dev<float>(o.X);
        D.first = G.dev<int32_t>(o.first); D.out_kf = G.dev<int32_t>(o.okf);
        D.out_idx1 = G.dev<int32_t>(o.oi1); D.out_idx2 = G.dev<int32_t>(o.oi2); D.out_x3d = G.dev<float>(o.ox);
        map_match_launch(st, D);
        map_triangulate_launch(st, D);
        map_resolve_launch(st, D);
        CCM_HIP(c, hipGetLastError());
        return map_finish(c, G, fn, o, n_kf, n1, cnode1.data(), hi2, res);
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
        int rc = frame_named_check(c, cur, CCM_E_ARG, fn, "current");       // an orphaned handle is CCM_E_ARG here, as it has always been
        if (rc) return rc;
        const int n1 = cur->n;
        for (int k = 0; k < n_kf; k++) {
            if (!pb->neighbours[k]) return ccm_fail(c, CCM_E_ARG, "%s: null neighbours[%d]", fn, k);
            if ((rc = frame_named_check(c, pb->neighbours[k], CCM_E_ARG, fn, "neighbours[%d]", k))) return rc;
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
        CCM_HIP(c, hipSetDevice(c->device));
        if (!c->map) c->map = new MapState();
        Staging& G = c->map->stage;

        // ---- staging: [MapKf | views] up, [per-pair work arrays] and [result list] down
        size_t off = 0;
        const size_t o_kf = seg(off, (size_t)n_kf * sizeof(MapKf)), o_view = seg(off, (size_t)(1 + n_kf) * sizeof(MapKfView));
        const MapOut o = map_out_layout(off, n_kf, n1);
        if ((rc = G.reserve(c, o.end))) return rc;
        MapKf* hkf = G.host<MapKf>(o_kf);
        MapKfView* hv = G.host<MapKfView>(o_view);
        hv[0] = view_of(cur);
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* kf = pb->neighbours[k];
            hv[1 + k] = view_of(kf);
            hkf[k].skipped = map_baseline_too_short(cur->cam.Ow, kf->cam.Ow, pb->median_depth[k]) ? 1 : 0;   // :319-328 on the handles' host copies
            hkf[k].ex = pb->epipole[2 * k]; hkf[k].ey = pb->epipole[2 * k + 1];
            std::memcpy(hkf[k].F12, pb->F12 + 9 * (size_t)k, 36);
        }
        if ((rc = G.upload(c, 0, o.in_end))) return rc;
        MapFramesDev D{};
        D.n1 = n1; D.n_kf = n_kf;
        D.ratioFactor = 1.5f * cur->sf1;                                     // :307
        D.kf = G.dev<MapKf>(o_kf); D.view = G.dev<MapKfView>(o_view);
        D.midx = G.dev<int32_t>(o.match); D.gate = G.dev<uint8_t>(o.gate); D.status = G.dev<uint8_t>(o.status); D.X = G.dev<float>(o.X);
        D.first = G.dev<int32_t>(o.first); D.out_kf = G.dev<int32_t>(o.okf);
        D.out_idx1 = G.dev<int32_t>(o.oi1); D.out_idx2 = G.dev<int32_t>(o.oi2); D.out_x3d = G.dev<float>(o.ox);
        map_frames_launch(c->stream, D);
        CCM_HIP(c, hipGetLastError());
        return map_finish(c, G, fn, o, n_kf, n1, nullptr, nullptr, res);
    });
}

// ---------------------------------------------------------------- the per-neighbour inputs, defined (no context, no GPU)
extern "C" int ccm_map_pair_geometry(const float K1[4], const float Tcw1[12], const float Ow1[3], const float K2[4], const float Tcw2[12],
                                     float F12[9], float epipole[2])
{
    if (!K1 || !Tcw1 || !Ow1 || !K2 || !Tcw2 || !F12 || !epipole) return CCM_E_ARG;
    map_pair_geometry(K1, Tcw1, Ow1, K2, Tcw2, F12, epipole);
    return CCM_OK;
}

extern "C" int ccm_scene_median_depth(int n, const int32_t* mp_id, int capacity, const float* pos, const uint8_t* flags, const float Tcw[12],
                                      float* median, int32_t* n_depths)
{
    if (n < 0 || capacity < 0 || (n > 0 && !mp_id) || (capacity > 0 && (!pos || !flags)) || !Tcw || !median || !n_depths) return CCM_E_ARG;
    try {
        float med = 0.0f;
        *n_depths = map_scene_median_depth(n, mp_id, capacity, pos, flags, Tcw, &med);
        *median = med;
        return CCM_OK;
    } catch (...) { return CCM_E_NOMEM; }
}
