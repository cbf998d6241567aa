// match_bow_host.cpp -- C ABI of the matchers that walk the vocabulary nodes (include/ccm_hot.h): ORBmatcher::SearchByBoW
// (cslam/src/ORBmatcher.cpp:178-306, 565-698; on the device, k_bow_greedy), on host arrays and on frame handles, and
// SearchForTriangulation (:700-852; distances from k_hamming_ranges, acceptance on the host).
#include "match_internal.h"
#include <algorithm>
#include <numeric>

extern "C" {

// The feature indices 0 .. n-1 by (node, index): the order of a DBoW2::FeatureVector walk
static std::vector<int> node_order(const int32_t* node, int n)
{
    std::vector<int> ord(n);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [node](int a, int b) { return node[a] != node[b] ? node[a] < node[b] : a < b; });
    return ord;
}

// Side-2 candidates of every side-1 feature = the features of the same vocabulary node (DBoW2::FeatureVector walk of
// SearchByBoW / SearchForTriangulation), with their Hamming distances from k_hamming_ranges.
struct BowRanges {
    std::vector<int> ord1, ord2, start, len;
    std::vector<long long> off;
    std::vector<unsigned short> dist;
};
static int bow_ranges(ccm_ctx* c, const uint8_t* desc1, const int32_t* node1, const uint8_t* valid1, int n1,
                      const uint8_t* desc2, const int32_t* node2, int n2, BowRanges& R)
{
    MatchState& M = *match_state(c);
    std::vector<int>&ord1 = R.ord1, &ord2 = R.ord2, &start = R.start, &len = R.len;
    std::vector<long long>& off = R.off;
    std::vector<unsigned short>& dist = R.dist;
    // FeatureVector order: node ascending, feature index ascending inside a node (DBoW2 fills it so)
    ord1 = node_order(node1, n1); ord2 = node_order(node2, n2);
    // per side-1 feature: the slice of ord2 holding its node (features without a node have id < 0)
    start.assign(n1, 0); len.assign(n1, 0); off.assign(n1 + 1, 0);
    {
        size_t b = 0;
        for (size_t a = 0; a < ord1.size();) {
            const int nd = node1[ord1[a]];
            size_t ae = a; while (ae < ord1.size() && node1[ord1[ae]] == nd) ae++;
            while (b < ord2.size() && node2[ord2[b]] < nd) b++;
            size_t be = b; while (be < ord2.size() && node2[ord2[be]] == nd) be++;
            if (nd >= 0) for (size_t i = a; i < ae; i++) if (valid1[ord1[i]]) { start[ord1[i]] = (int)b; len[ord1[i]] = (int)(be - b); }
            a = ae; b = be;
        }
    }
    for (int i = 0; i < n1; i++) off[i + 1] = off[i] + len[i];
    const long long total = off[n1];
    dist.assign((size_t)std::max<long long>(total, 1), 0);
    if (total > 0) {
        CCM_RESERVE(c, M.d1, (size_t)n1 * 32); CCM_RESERVE(c, M.d2, (size_t)n2 * 32);
        CCM_RESERVE(c, M.order2, (size_t)n2 * 4); CCM_RESERVE(c, M.start, (size_t)n1 * 4); CCM_RESERVE(c, M.len, (size_t)n1 * 4);
        CCM_RESERVE(c, M.off, (size_t)(n1 + 1) * 8); CCM_RESERVE(c, M.dist, (size_t)total * 2);
        CCM_HIP(c, hipMemcpyAsync(M.d1.p, desc1, (size_t)n1 * 32, hipMemcpyHostToDevice, c->stream));
        CCM_HIP(c, hipMemcpyAsync(M.d2.p, desc2, (size_t)n2 * 32, hipMemcpyHostToDevice, c->stream));
        CCM_HIP(c, hipMemcpyAsync(M.order2.p, ord2.data(), (size_t)n2 * 4, hipMemcpyHostToDevice, c->stream));
        CCM_HIP(c, hipMemcpyAsync(M.start.p, start.data(), (size_t)n1 * 4, hipMemcpyHostToDevice, c->stream));
        CCM_HIP(c, hipMemcpyAsync(M.len.p, len.data(), (size_t)n1 * 4, hipMemcpyHostToDevice, c->stream));
        CCM_HIP(c, hipMemcpyAsync(M.off.p, off.data(), (size_t)(n1 + 1) * 8, hipMemcpyHostToDevice, c->stream));
        match_launch_ranges(c->stream, M.d1.as<uint8_t>(), M.d2.as<uint8_t>(), M.order2.as<int>(), M.start.as<int>(),
                            M.len.as<int>(), M.off.as<long long>(), n1, M.dist.as<unsigned short>());
        CCM_HIP(c, hipGetLastError());
        CCM_HIP(c, hipMemcpyAsync(dist.data(), M.dist.p, (size_t)total * 2, hipMemcpyDeviceToHost, c->stream));
        CCM_HIP(c, hipStreamSynchronize(c->stream));
    }
    return CCM_OK;
}

int ccm_match_bow(ccm_ctx* c, const ccm_bow_options* o, const uint8_t* desc1, const int32_t* node1, const uint8_t* valid1,
                  const float* angle1, int n1, const uint8_t* desc2, const int32_t* node2, const uint8_t* valid2,
                  const float* angle2, int n2, int32_t* match12)
{
    RoctxRange roctx_("ccm_match_bow");
    return ccm_guard(c, "ccm_match_bow", [&]() -> int {
        if (!c || !o) return CCM_E_ARG;
        if (n1 < 0 || n2 < 0 || (n1 > 0 && (!desc1 || !node1 || !valid1 || !match12)) || (n2 > 0 && (!desc2 || !node2)) ||
            (o->check_ori && n1 > 0 && n2 > 0 && (!angle1 || !angle2)))
            return ccm_fail(c, CCM_E_ARG, "bad SearchByBoW arguments");
        for (int i = 0; i < n1; i++) match12[i] = -1;
        if (n1 == 0 || n2 == 0) return 0;
        CCM_HIP(c, hipSetDevice(c->device));
        MatchState& M = *match_state(c);
        // FeatureVector order: node ascending, feature index ascending inside a node (DBoW2 fills it so); the merge walk of
        // :201-298 pairs the runs of equal node ids -- one group per common node
        const std::vector<int> ord1 = node_order(node1, n1), ord2 = node_order(node2, n2);
        std::vector<int> grp[4];
        {
            size_t pa = 0, pb = 0;
            while (pa < ord1.size() && pb < ord2.size()) {
                const int na = node1[ord1[pa]], nb2 = node2[ord2[pb]];
                if (na < 0) { pa++; continue; }                              // features without a node are in no FeatureVector entry
                if (nb2 < 0) { pb++; continue; }
                if (na < nb2) { while (pa < ord1.size() && node1[ord1[pa]] == na) pa++; continue; }
                if (nb2 < na) { while (pb < ord2.size() && node2[ord2[pb]] == nb2) pb++; continue; }
                size_t ae = pa, be = pb;
                while (ae < ord1.size() && node1[ord1[ae]] == na) ae++;
                while (be < ord2.size() && node2[ord2[be]] == na) be++;
                grp[0].push_back((int)pa); grp[1].push_back((int)ae); grp[2].push_back((int)pb); grp[3].push_back((int)be);
                pa = ae; pb = be;
            }
        }
        const int ng = (int)grp[0].size();
        hipStream_t st = c->stream;
        int rc;
        if ((rc = ccm_upload(c, M.d1, desc1, (size_t)n1 * 32, st)) || (rc = ccm_upload(c, M.d2, desc2, (size_t)n2 * 32, st))) return rc;
        if ((rc = ccm_upload(c, M.order1, ord1.data(), (size_t)n1 * 4, st)) || (rc = ccm_upload(c, M.order2, ord2.data(), (size_t)n2 * 4, st))) return rc;
        for (int k = 0; k < 4; k++) if ((rc = ccm_upload(c, M.grp[k], grp[k].data(), (size_t)ng * 4, st))) return rc;
        if ((rc = ccm_upload(c, M.bv1, valid1, (size_t)n1, st))) return rc;
        if (valid2 && (rc = ccm_upload(c, M.bv2, valid2, (size_t)n2, st))) return rc;
        if (o->check_ori && ((rc = ccm_upload(c, M.ba1, angle1, (size_t)n1 * 4, st)) || (rc = ccm_upload(c, M.ba2, angle2, (size_t)n2 * 4, st)))) return rc;
        CCM_RESERVE(c, M.taken, (size_t)n2); CCM_RESERVE(c, M.m12, (size_t)n1 * 4); CCM_RESERVE(c, M.binof, (size_t)n1 * 4); CCM_RESERVE(c, M.hist, 32 * 4);
        CCM_HIP(c, hipMemsetAsync(M.taken.p, 0, (size_t)n2, st));
        CCM_HIP(c, hipMemsetAsync(M.m12.p, 0xFF, (size_t)n1 * 4, st));
        CCM_HIP(c, hipMemsetAsync(M.hist.p, 0, 32 * 4, st));
        BowDev B{ ng, n1, M.grp[0].as<int>(), M.grp[1].as<int>(), M.grp[2].as<int>(), M.grp[3].as<int>(), M.order1.as<int>(), M.order2.as<int>(),
                  M.d1.as<uint8_t>(), M.d2.as<uint8_t>(), M.bv1.as<uint8_t>(), valid2 ? M.bv2.as<uint8_t>() : nullptr,
                  M.ba1.as<float>(), M.ba2.as<float>(), M.taken.as<uint8_t>(), M.m12.as<int>(), M.binof.as<int>(), M.hist.as<int>(),
                  o->nnratio, o->th, o->strict_th, o->check_ori };
        match_launch_bow(st, B);
        CCM_HIP(c, hipGetLastError());
        int nmatches = 0;
        CCM_HIP(c, hipMemcpyAsync(match12, M.m12.p, (size_t)n1 * 4, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipMemcpyAsync(&nmatches, M.hist.as<int>() + 30, 4, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipStreamSynchronize(st));
        return nmatches;
    });
}

// ---- SearchByBoW on frame handles.  Both sides carry descriptors, angles, mp_id and the node directory in device memory: the group
// list is made by k_bow_groups, k_bow_greedy / k_bow_filter run on the handles' arrays, and a call costs at most one upload (the
// caller's masks, with the pair records of the batch), one download and one synchronisation.
static int bow_handle_check(ccm_ctx* c, const ccm_frame* f, const char* fn, const char* who, int k, int check_ori)
{
    char name[48];
    if (k >= 0) snprintf(name, sizeof name, "%s[%d]", who, k); else snprintf(name, sizeof name, "%s", who);
    const int rc = frame_named_check(c, f, CCM_E_STATE, fn, "%s", name);
    if (rc) return rc;
    if (!f->has_bow) return ccm_fail(c, CCM_E_STATE, "%s: %s has no bow", fn, name);
    if (check_ori && !f->has_angle) return ccm_fail(c, CCM_E_ARG, "%s: orientation check against %s, created without angles", fn, name);
    return CCM_OK;
}

// ORBmatcher::SearchByBoW(KeyFrame, Frame), ORBmatcher.cpp:178-306, as Tracking::TrackReferenceKeyFrame calls it (src/Tracking.cpp:514-529)
int ccm_frame_search_by_bow(ccm_ctx* c, const ccm_frame* kf, ccm_frame* f, const ccm_bow_options* o, const uint8_t* valid1, int min_matches,
                            int32_t* match)
{
    RoctxRange roctx_("ccm_frame_search_by_bow");
    static const char* fn = "ccm_frame_search_by_bow";
    if (!c || !o) return CCM_E_ARG;
    int rc;
    if ((rc = bow_handle_check(c, kf, fn, "kf", -1, o->check_ori)) || (rc = bow_handle_check(c, f, fn, "f", -1, o->check_ori))) return rc;
    if (kf == f) return ccm_fail(c, CCM_E_ARG, "%s: kf and f are the same handle", fn);
    if (f->n > 0 && !match) return ccm_fail(c, CCM_E_ARG, "%s: null match", fn);
    return ccm_guard(c, fn, [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        MatchState& M = *match_state(c);
        hipStream_t st = c->stream;
        const int n1 = kf->n, n2 = f->n, ng = kf->n_nodes;
        size_t off = 0;
        const size_t o_hist = seg(off, 32 * 4), o_m21 = seg(off, (size_t)n2 * 4);
        const size_t res_end = o_m21 + (size_t)n2 * 4;
        const size_t o_v1 = seg(off, valid1 ? (size_t)n1 : 0);
        const size_t end = off;
        Staging& G = frame_state(c)->stage;
        if ((rc = G.reserve(c, end))) return rc;
        if (valid1) {
            G.put(o_v1, valid1, (size_t)n1);
            if ((rc = G.upload(c, o_v1, o_v1 + (size_t)n1))) return rc;
        }
        size_t t = 0;
        const size_t t_grp = seg(t, 4 * (size_t)ng * 4), t_taken = seg(t, (size_t)n2), t_m12 = seg(t, (size_t)n1 * 4), t_bin = seg(t, (size_t)n1 * 4);
        const size_t t_v1 = seg(t, (size_t)n1);
        CCM_RESERVE(c, M.bowf, std::max<size_t>(t, 64));
        uint8_t* tmp = M.bowf.as<uint8_t>();
        int* grp = (int*)(tmp + t_grp);
        uint8_t* v1 = valid1 ? G.dev<uint8_t>(o_v1) : tmp + t_v1;
        BowFrameRec R{};
        R.B = BowDev{ ng, n1, grp, grp + ng, grp + 2 * ng, grp + 3 * ng, kf->order, f->order, kf->desc, f->desc, v1, nullptr, kf->angle, f->angle,
                      tmp + t_taken, (int*)(tmp + t_m12), (int*)(tmp + t_bin), G.dev<int>(o_hist), o->nnratio, o->th, o->strict_th, o->check_ori };
        R.nodes1 = kf->nodes; R.first1 = kf->first; R.nodes2 = f->nodes; R.first2 = f->first; R.n_nodes2 = f->n_nodes; R.n2 = n2;
        R.mp1 = kf->mp_id; R.mp2 = f->mp_id; R.v1 = valid1 ? nullptr : v1; R.v2 = nullptr; R.match21 = G.dev<int>(o_m21);
        match_launch_bow_groups(st, R, nullptr, 1, std::max(std::max(ng, n1), n2));
        match_launch_bow(st, R.B);
        match_launch_bow_invert(st, R, min_matches, f->mp_id);
        CCM_HIP(c, hipGetLastError());
        if ((rc = G.download(c, 0, res_end)) || (rc = G.wait(c))) return rc;
        int nmatches = 0;
        G.get(&nmatches, o_hist + 30 * 4, 4);
        G.get(match, o_m21, (size_t)n2 * 4);
        return nmatches;
    });
}

// ORBmatcher::SearchByBoW(KeyFrame, KeyFrame), ORBmatcher.cpp:565-698, for one keyframe against every candidate of
// LoopFinder::ComputeSim3 (src/LoopFinder.cpp:265) / MapMatcher (src/MapMatcher.cpp:271) at once
int ccm_search_by_bow_frames(ccm_ctx* c, const ccm_frame* kf1, int n_kf2, ccm_frame* const* kfs2, const ccm_bow_options* o, const uint8_t* valid1,
                             const int32_t* first2, const uint8_t* valid2, int32_t* match12, int32_t* nmatches)
{
    RoctxRange roctx_("ccm_search_by_bow_frames");
    static const char* fn = "ccm_search_by_bow_frames";
    if (!c || !o) return CCM_E_ARG;
    int rc;
    if ((rc = bow_handle_check(c, kf1, fn, "kf1", -1, o->check_ori))) return rc;
    if (n_kf2 < 0 || n_kf2 > 65535) return ccm_fail(c, CCM_E_ARG, "%s: n_kf2 = %d outside [0, 65535]", fn, n_kf2);
    if (n_kf2 == 0) return CCM_OK;
    if (!kfs2 || !nmatches || (kf1->n > 0 && !match12) || (valid2 && !first2)) return ccm_fail(c, CCM_E_ARG, "%s: null argument", fn);
    for (int k = 0; k < n_kf2; k++) {
        if ((rc = bow_handle_check(c, kfs2[k], fn, "kfs2", k, o->check_ori))) return rc;
        if (first2 && first2[k + 1] - first2[k] != kfs2[k]->n)
            return ccm_fail(c, CCM_E_ARG, "%s: first2[%d..] spans %d entries, kfs2[%d] has %d features", fn, k, first2[k + 1] - first2[k], k, kfs2[k]->n);
    }
    return ccm_guard(c, fn, [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        MatchState& M = *match_state(c);
        hipStream_t st = c->stream;
        const int n1 = kf1->n, ng = kf1->n_nodes;
        std::vector<size_t> at2((size_t)n_kf2 + 1, 0);                          // offsets of the candidates' features, concatenated
        int max_n2 = 0;
        for (int k = 0; k < n_kf2; k++) { at2[k + 1] = at2[k] + (size_t)kfs2[k]->n; max_n2 = std::max(max_n2, kfs2[k]->n); }
        size_t off = 0;
        const size_t o_hist = seg(off, (size_t)n_kf2 * 32 * 4), o_m12 = seg(off, (size_t)n_kf2 * n1 * 4);
        const size_t res_end = o_m12 + (size_t)n_kf2 * n1 * 4;
        const size_t o_rec = seg(off, (size_t)n_kf2 * sizeof(BowFrameRec)), o_v1 = seg(off, valid1 ? (size_t)n1 : 0);
        const size_t o_v2 = seg(off, valid2 ? at2[n_kf2] : 0);
        const size_t end = off;
        Staging& G = frame_state(c)->stage;
        if ((rc = G.reserve(c, end))) return rc;
        size_t t = 0;
        const size_t t_grp = seg(t, (size_t)n_kf2 * 4 * ng * 4), t_taken = seg(t, at2[n_kf2]), t_bin = seg(t, (size_t)n_kf2 * n1 * 4);
        const size_t t_v1 = seg(t, (size_t)n1), t_v2 = seg(t, at2[n_kf2]);
        CCM_RESERVE(c, M.bowf, std::max<size_t>(t, 64));
        uint8_t* tmp = M.bowf.as<uint8_t>();
        uint8_t* v1 = valid1 ? G.dev<uint8_t>(o_v1) : tmp + t_v1;
        BowFrameRec* recs = G.host<BowFrameRec>(o_rec);
        for (int k = 0; k < n_kf2; k++) {
            const ccm_frame* f = kfs2[k];
            int* grp = (int*)(tmp + t_grp) + (size_t)k * 4 * ng;
            uint8_t* v2 = valid2 ? G.dev<uint8_t>(o_v2 + at2[k]) : tmp + t_v2 + at2[k];
            BowFrameRec R{};
            R.B = BowDev{ ng, n1, grp, grp + ng, grp + 2 * ng, grp + 3 * ng, kf1->order, f->order, kf1->desc, f->desc, v1, v2, kf1->angle, f->angle,
                          tmp + t_taken + at2[k], G.dev<int>(o_m12) + (size_t)k * n1, (int*)(tmp + t_bin) + (size_t)k * n1,
                          G.dev<int>(o_hist) + (size_t)k * 32, o->nnratio, o->th, 1, o->check_ori };
            R.nodes1 = kf1->nodes; R.first1 = kf1->first; R.nodes2 = f->nodes; R.first2 = f->first; R.n_nodes2 = f->n_nodes; R.n2 = f->n;
            R.mp1 = kf1->mp_id; R.mp2 = f->mp_id; R.v1 = valid1 ? nullptr : v1; R.v2 = valid2 ? nullptr : v2; R.match21 = nullptr;
            std::memcpy(recs + k, &R, sizeof R);
        }
        G.put(o_v1, valid1, (size_t)n1);
        if (valid2) for (int k = 0; k < n_kf2; k++) G.put(o_v2 + at2[k], valid2 + first2[k], (size_t)kfs2[k]->n);
        if ((rc = G.upload(c, o_rec, end))) return rc;
        const BowFrameRec* d_recs = G.dev<BowFrameRec>(o_rec);
        match_launch_bow_groups(st, BowFrameRec{}, d_recs, n_kf2, std::max(std::max(ng, n1), max_n2));
        match_launch_bow_batch(st, d_recs, n_kf2, ng);
        CCM_HIP(c, hipGetLastError());
        if ((rc = G.download(c, 0, res_end)) || (rc = G.wait(c))) return rc;
        for (int k = 0; k < n_kf2; k++) G.get(nmatches + k, o_hist + ((size_t)k * 32 + 30) * 4, 4);
        G.get(match12, o_m12, (size_t)n_kf2 * n1 * 4);
        return CCM_OK;
    });
}

// ORBmatcher::CheckDistEpipolarLine, ORBmatcher.cpp:159-176
static bool check_dist_epipolar_line(float x1, float y1, float x2, float y2, const float* F12, float sigma2)
{
    const float a = x1 * F12[0] + y1 * F12[3] + F12[6];
    const float b = x1 * F12[1] + y1 * F12[4] + F12[7];
    const float cc = x1 * F12[2] + y1 * F12[5] + F12[8];
    const float num = a * x2 + b * y2 + cc;
    const float den = a * a + b * b;
    if (den == 0) return false;
    const float dsqr = num * num / den;
    return dsqr < 3.84 * sigma2;
}

// ORBmatcher::SearchForTriangulation, ORBmatcher.cpp:700-852
int ccm_search_for_triangulation(ccm_ctx* c, const uint8_t* desc1, const int32_t* node1, const uint8_t* has_mp1, const float* x1, const float* y1,
                                 const float* angle1, int n1, const uint8_t* desc2, const int32_t* node2, const uint8_t* has_mp2,
                                 const float* x2, const float* y2, const float* angle2, const int32_t* octave2, int n2, const float* F12,
                                 float ex, float ey, const float* scale_factors2, const float* level_sigma2_2, int check_ori, int32_t* match12)
{
    return ccm_guard(c, "ccm_search_for_triangulation", [&]() -> int {
        if (!c) return CCM_E_ARG;
        if (n1 < 0 || n2 < 0 || (n1 > 0 && (!desc1 || !node1 || !has_mp1 || !x1 || !y1 || !match12 || (check_ori && !angle1))) ||
            (n2 > 0 && (!desc2 || !node2 || !has_mp2 || !x2 || !y2 || !octave2 || (check_ori && !angle2))) || !F12 || !scale_factors2 || !level_sigma2_2)
            return ccm_fail(c, CCM_E_ARG, "bad SearchForTriangulation arguments");
        for (int i = 0; i < n1; i++) match12[i] = -1;
        if (n1 == 0 || n2 == 0) return 0;
        CCM_HIP(c, hipSetDevice(c->device));
        std::vector<uint8_t> free1(n1);
        for (int i = 0; i < n1; i++) free1[i] = !has_mp1[i];                                         // :744-746
        BowRanges R;
        int rc = bow_ranges(c, desc1, node1, free1.data(), n1, desc2, node2, n2, R);
        if (rc) return rc;
        RotHisto rot;
        int nmatches = 0;
        for (int i1 : R.ord1) {
            if (node1[i1] < 0 || !free1[i1] || R.len[i1] == 0) continue;
            int bestDist = 50, bestIdx2 = -1;                                                       // TH_LOW
            const unsigned short* d = R.dist.data() + R.off[i1];
            for (int k = 0; k < R.len[i1]; k++) {
                const int idx2 = R.ord2[R.start[i1] + k];
                if (has_mp2[idx2]) continue;                                                         // :763; vbMatched2 is never set
                const int dist = d[k];
                if (dist > 50 || dist > bestDist) continue;
                const float distex = ex - x2[idx2], distey = ey - y2[idx2];
                if (distex * distex + distey * distey < 100 * scale_factors2[octave2[idx2]]) continue;
                if (check_dist_epipolar_line(x1[i1], y1[i1], x2[idx2], y2[idx2], F12, level_sigma2_2[octave2[idx2]])) { bestIdx2 = idx2; bestDist = dist; }
            }
            if (bestIdx2 >= 0) {
                match12[i1] = bestIdx2;
                nmatches++;
                if (check_ori) rot.add(angle1[i1] - angle2[bestIdx2], i1);
            }
        }
        if (check_ori) for (int idx : rot.outliers()) { match12[idx] = -1; nmatches--; }
        return nmatches;
    });
}

}  // extern "C"
