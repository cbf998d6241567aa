// match_window_host.cpp -- C ABI of the windowed matchers (include/ccm_hot.h) and their host pieces that window_types.h declares.
#include "match_internal.h"
#include <algorithm>
#include <climits>
#include <cmath>

// F1: windowed matching.  The GPU enumerates, for every query, the features inside its
// search window with their Hamming distances (k_window_candidates).  The acceptance runs on the device too for the matchers
// a server batches over many map points: Fuse / SearchBySim3 (k_window_select: no coupling between queries), and
// SearchByProjection(Frame, map points) / SearchByProjection(KF, Scw) / SearchByProjection(Frame, Frame | KeyFrame)
// (k_window_greedy: the reference's order-dependent occupancy bookkeeping resolved by claim rounds, bit-identical to the
// sequential loop; the frame matcher's rotation histogram and its three maxima in the same kernel).  Only the
// initialisation matcher (called once per map) keeps its acceptance loop on the host.

// Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cpp:103-118, 255-266) for one grid: mGrid[x][y] is cell x * rows + y, its
// features cell_items[cell_first[cell] .. cell_first[cell + 1]) in index order.  cell_first has cols * rows + 1 entries, cell_items f.n.
static void grid_build(const ccm_frame_grid& f, int* cell_first, int* cell_items)
{
    const int n = f.n, cells = f.grid_cols * f.grid_rows;
    std::vector<int> cell(n);
    for (int k = 0; k <= cells; k++) cell_first[k] = 0;
    for (int i = 0; i < n; i++) {
        const int px = (int)std::round((f.kp_x[i] - f.min_x) * f.inv_w), py = (int)std::round((f.kp_y[i] - f.min_y) * f.inv_h);
        cell[i] = (px < 0 || px >= f.grid_cols || py < 0 || py >= f.grid_rows) ? -1 : px * f.grid_rows + py;
        if (cell[i] >= 0) cell_first[cell[i] + 1]++;
    }
    for (int k = 0; k < cells; k++) cell_first[k + 1] += cell_first[k];
    std::vector<int> fill(cell_first, cell_first + std::max(cells, 0));
    for (int i = 0; i < n; i++) if (cell[i] >= 0) cell_items[fill[cell[i]]++] = i;
}

// The queries of a call into the context's WindowBufs.  L: the call on its lists in W.ci / cd / cn, over the one frame G or, with qkf
// (each query's keyframe), over the batch's WinGrid table in W.grids.
static int window_stage_queries(ccm_ctx* c, const WinGrid& G, int nq, const float* qx, const float* qy, const float* qr, const int32_t* minl,
                                const int32_t* maxl, const uint8_t* qdesc, const int32_t* qkf, WinLists& L)
{
    WindowBufs& W = window_bufs(c);
    hipStream_t st = c->stream;
    int rc;
    if ((rc = ccm_upload(c, W.qx, qx, (size_t)nq * 4, st)) || (rc = ccm_upload(c, W.qy, qy, (size_t)nq * 4, st)) ||
        (rc = ccm_upload(c, W.qr, qr, (size_t)nq * 4, st)) || (rc = ccm_upload(c, W.minl, minl, (size_t)nq * 4, st)) ||
        (rc = ccm_upload(c, W.maxl, maxl, (size_t)nq * 4, st)) || (rc = ccm_upload(c, W.qdesc, qdesc, (size_t)nq * 32, st)) ||
        (qkf && (rc = ccm_upload(c, W.qkf, qkf, (size_t)nq * 4, st))))
        return rc;
    L = WinLists{ G, qkf ? W.grids.as<WinGrid>() : nullptr, W.qkf.as<int>(), nq, W.qx.as<float>(), W.qy.as<float>(), W.qr.as<float>(), W.minl.as<int>(),
                  W.maxl.as<int>(), W.qdesc.as<uint8_t>(), &W.ci, &W.cd, &W.cn };
    return CCM_OK;
}

// A frame (its grid built here) and its queries into WindowBufs, once per call
static int window_stage(ccm_ctx* c, const ccm_frame_grid* f, int nq, const float* qx, const float* qy, const float* qr, const int32_t* minl,
                        const int32_t* maxl, const uint8_t* qdesc, WinLists& L)
{
    WindowBufs& W = window_bufs(c);
    const int n = f->n;
    std::vector<int> first(f->grid_cols * f->grid_rows + 1), items(std::max(n, 1));
    grid_build(*f, first.data(), items.data());
    hipStream_t st = c->stream;
    int rc;
    if ((rc = ccm_upload(c, W.kx, f->kp_x, (size_t)n * 4, st)) || (rc = ccm_upload(c, W.ky, f->kp_y, (size_t)n * 4, st)) ||
        (rc = ccm_upload(c, W.oct, f->kp_octave, (size_t)n * 4, st)) || (rc = ccm_upload(c, W.desc, f->desc, (size_t)n * 32, st)) ||
        (rc = ccm_upload(c, W.cfirst, first.data(), first.size() * 4, st)) || (rc = ccm_upload(c, W.citems, items.data(), (size_t)n * 4, st)))
        return rc;
    const WinGrid G{ n, f->grid_cols, f->grid_rows, f->min_x, f->min_y, f->inv_w, f->inv_h, W.kx.as<float>(), W.ky.as<float>(), W.oct.as<int>(),
                     W.desc.as<uint8_t>(), W.cfirst.as<int>(), W.citems.as<int>() };
    return window_stage_queries(c, G, nq, qx, qy, qr, minl, maxl, qdesc, nullptr, L);
}

int window_lists_launch(ccm_ctx* c, const WinLists& L, int cap)
{
    CCM_RESERVE(c, *L.ci, (size_t)L.nq * cap * 4); CCM_RESERVE(c, *L.cd, (size_t)L.nq * cap * 4); CCM_RESERVE(c, *L.cn, (size_t)L.nq * 4);
    if (L.grids)
        match_launch_window_batch(c->stream, L.grids, L.q_kf, L.nq, L.qx, L.qy, L.qr, L.minl, L.maxl, L.qdesc, cap, L.ci->as<int>(), L.cd->as<int>(), L.cn->as<int>());
    else
        match_launch_window(c->stream, L.grid, L.nq, L.qx, L.qy, L.qr, L.minl, L.maxl, L.qdesc, cap, L.ci->as<int>(), L.cd->as<int>(), L.cn->as<int>());
    CCM_HIP(c, hipGetLastError());
    return CCM_OK;
}

// The lists of a launch at `cap` into host arrays of [nq][cap], [nq][cap] and [nq]
static int window_lists_fetch(ccm_ctx* c, const WinLists& L, int cap, int32_t* ci, int32_t* cd, int32_t* cn)
{
    CCM_HIP(c, hipMemcpyAsync(ci, L.ci->p, (size_t)L.nq * cap * 4, hipMemcpyDeviceToHost, c->stream));
    CCM_HIP(c, hipMemcpyAsync(cd, L.cd->p, (size_t)L.nq * cap * 4, hipMemcpyDeviceToHost, c->stream));
    CCM_HIP(c, hipMemcpyAsync(cn, L.cn->p, (size_t)L.nq * 4, hipMemcpyDeviceToHost, c->stream));
    CCM_HIP(c, hipStreamSynchronize(c->stream));
    return CCM_OK;
}

int window_lists_host(ccm_ctx* c, const WinLists& L, WinHostLists& H)
{
    H.cn.resize(L.nq);
    for (;;) {
        H.ci.resize((size_t)L.nq * H.cap); H.cd.resize((size_t)L.nq * H.cap);
        int rc, mx = 0;
        if ((rc = window_lists_launch(c, L, H.cap)) || (rc = window_lists_fetch(c, L, H.cap, H.ci.data(), H.cd.data(), H.cn.data()))) return rc;
        for (int v : H.cn) mx = std::max(mx, v);
        if (mx <= H.cap) return CCM_OK;
        H.cap = mx;
    }
}

// The order-dependent acceptance on the device (k_window_greedy) for staged queries.  in: per-query active / level / flag and the
// n_flag per-feature flags; out: `out` (n_out ints, -1 where nothing is chosen), the updated flags and, for a batch (kfs [n_problems],
// frames of at most max_n features), the matches of each problem in n_matches.  Returns the match count, or < 0 on error.
static int window_greedy(ccm_ctx* c, const WinLists& L, int mode, const uint8_t* active, const int32_t* qlevel, const uint8_t* qflag, uint8_t* flag,
                         int n_flag, float nnratio, int32_t* out, int n_out, int orb_dist = 0, int check_ori = 0, const float* q_angle = nullptr,
                         const float* f_angle = nullptr, const std::vector<GreedyKf>* kfs = nullptr, int max_n = 0, int32_t* n_matches = nullptr)
{
    WindowBufs& W = window_bufs(c);
    hipStream_t st = c->stream;
    const int nq = L.nq, n_problems = kfs ? (int)kfs->size() : 1;
    int rc;
    if ((rc = ccm_upload(c, W.act, active, (size_t)nq, st)) || (rc = ccm_upload(c, W.qflag, qflag, (size_t)nq, st))) return rc;
    if (qlevel && (rc = ccm_upload(c, W.qlvl, qlevel, (size_t)nq * 4, st))) return rc;
    if (kfs && (rc = ccm_upload(c, W.gkf, kfs->data(), kfs->size() * sizeof(GreedyKf), st))) return rc;
    if (mode == 2) {
        CCM_RESERVE(c, W.ev, std::max<size_t>((size_t)nq * 4, 16));
        if (check_ori && ((rc = ccm_upload(c, W.qang, q_angle, (size_t)nq * 4, st)) || (rc = ccm_upload(c, W.fang, f_angle, (size_t)n_flag * 4, st))))
            return rc;
    }
    CCM_RESERVE(c, W.out, std::max<size_t>((size_t)n_out * 4, 16)); CCM_RESERVE(c, W.status, (size_t)n_problems * 12 + 16);
    auto reset = [&]() -> int {                                                  // the flags and choices as they come in
        if (int e = ccm_upload(c, W.flag, flag, (size_t)n_flag, st)) return e;
        CCM_HIP(c, hipMemsetAsync(W.out.p, 0xFF, (size_t)n_out * 4, st));
        return CCM_OK;
    };
    if ((rc = reset())) return rc;
    GreedyArgs A{ kfs ? 0 : nq, kfs ? 0 : n_flag, 0, nullptr, nullptr, nullptr, W.act.as<uint8_t>(), qlevel ? W.qlvl.as<int>() : nullptr, W.oct.as<int>(),
                  W.qflag.as<uint8_t>(), W.flag.as<uint8_t>(), nnratio, W.out.as<int>(), W.status.as<int>(), orb_dist, check_ori, W.qang.as<float>(),
                  W.fang.as<float>(), W.ev.as<int>(), kfs ? W.gkf.as<GreedyKf>() : nullptr };
    std::vector<int> words(3 * (size_t)n_problems);
    const int* status = nullptr;
    auto fetch = [&](const int** s) -> int {                                     // the status words alone; the results follow a success
        *s = words.data();
        CCM_HIP(c, hipMemcpyAsync(words.data(), W.status.p, words.size() * 4, hipMemcpyDeviceToHost, st));
        CCM_HIP(c, hipStreamSynchronize(st));
        return CCM_OK;
    };
    if ((rc = window_greedy_drive(c, L, A, mode, n_problems, max_n, reset, [] {}, fetch, &status))) return rc;
    CCM_HIP(c, hipMemcpyAsync(out, W.out.p, (size_t)n_out * 4, hipMemcpyDeviceToHost, st));
    CCM_HIP(c, hipMemcpyAsync(flag, W.flag.p, (size_t)n_flag, hipMemcpyDeviceToHost, st));
    CCM_HIP(c, hipStreamSynchronize(st));
    int total = 0;
    for (int k = 0; k < n_problems; k++) { if (n_matches) n_matches[k] = status[3 * k]; total += status[3 * k]; }
    return total;
}

// The keyframes of a batch call, concatenated: keyframe k's features are rows feat_first[k] .. feat_first[k + 1] - 1 of W.kx / ky /
// oct / desc / citems (its items index its own features), W.grids[k] is its WinGrid.  The host arrays stay alive with the KfBatch
// until the caller's stream synchronisation.  n_levels: 1 + the largest octave.
struct KfBatch {
    std::vector<int> feat_first, oct, items, cfirst;
    std::vector<float> kx, ky;
    std::vector<uint8_t> desc;
    std::vector<WinGrid> grids;
    int n_levels = 1;
};
static int stage_keyframes(ccm_ctx* c, int n_kf, const ccm_frame_grid* kfs, KfBatch& B)
{
    WindowBufs& W = window_bufs(c);
    std::vector<int> cell_first_off(n_kf + 1, 0);
    B.feat_first.assign(n_kf + 1, 0);
    for (int k = 0; k < n_kf; k++) {
        B.feat_first[k + 1] = B.feat_first[k] + kfs[k].n;
        cell_first_off[k + 1] = cell_first_off[k] + kfs[k].grid_cols * kfs[k].grid_rows + 1;
    }
    const int NF = B.feat_first[n_kf];
    const size_t m = (size_t)std::max(NF, 1);
    B.kx.resize(m); B.ky.resize(m); B.oct.resize(m); B.items.resize(m); B.desc.resize(m * 32); B.cfirst.resize(cell_first_off[n_kf]);
    for (int k = 0; k < n_kf; k++) {
        const ccm_frame_grid& f = kfs[k];
        const int f0 = B.feat_first[k];
        grid_build(f, B.cfirst.data() + cell_first_off[k], B.items.data() + f0);
        std::copy(f.kp_x, f.kp_x + f.n, B.kx.begin() + f0); std::copy(f.kp_y, f.kp_y + f.n, B.ky.begin() + f0);
        std::copy(f.kp_octave, f.kp_octave + f.n, B.oct.begin() + f0); std::copy(f.desc, f.desc + (size_t)f.n * 32, B.desc.begin() + (size_t)f0 * 32);
        for (int i = 0; i < f.n; i++) B.n_levels = std::max(B.n_levels, f.kp_octave[i] + 1);
    }
    hipStream_t st = c->stream;
    int rc;
    if ((rc = ccm_upload(c, W.kx, B.kx.data(), (size_t)NF * 4, st)) || (rc = ccm_upload(c, W.ky, B.ky.data(), (size_t)NF * 4, st)) ||
        (rc = ccm_upload(c, W.oct, B.oct.data(), (size_t)NF * 4, st)) || (rc = ccm_upload(c, W.desc, B.desc.data(), (size_t)NF * 32, st)) ||
        (rc = ccm_upload(c, W.cfirst, B.cfirst.data(), B.cfirst.size() * 4, st)) || (rc = ccm_upload(c, W.citems, B.items.data(), (size_t)NF * 4, st)))
        return rc;
    B.grids.resize(n_kf);
    for (int k = 0; k < n_kf; k++) {
        const ccm_frame_grid& f = kfs[k];
        const int f0 = B.feat_first[k];
        B.grids[k] = WinGrid{ f.n, f.grid_cols, f.grid_rows, f.min_x, f.min_y, f.inv_w, f.inv_h, W.kx.as<float>() + f0, W.ky.as<float>() + f0,
                              W.oct.as<int>() + f0, W.desc.as<uint8_t>() + (size_t)f0 * 32, W.cfirst.as<int>() + cell_first_off[k], W.citems.as<int>() + f0 };
    }
    return ccm_upload(c, W.grids, B.grids.data(), B.grids.size() * sizeof(WinGrid), st);
}

bool window_host_accept_forced()
{
    static const bool host_accept = getenv("CCM_WINDOW_HOST_ACCEPT") && atoi(getenv("CCM_WINDOW_HOST_ACCEPT")) != 0;   // test switch
    return host_accept;
}

WinQueries window_queries_projection(int n_mp, const uint8_t* in_view, const int32_t* level, const float* view_cos, const float* scale_factors,
                                     float th)
{
    const bool bFactor = th != 1.0;
    WinQueries q{ std::vector<float>(n_mp), std::vector<int32_t>(n_mp), std::vector<int32_t>(n_mp) };
    for (int m = 0; m < n_mp; m++) {
        if (!in_view[m]) { q.qr[m] = -1.f; q.minl[m] = 0; q.maxl[m] = 0; continue; }
        float r = view_cos[m] > 0.998 ? 2.5f : 4.0f;                          // RadiusByViewingCos :150-156
        if (bFactor) r *= th;
        q.qr[m] = r * scale_factors[level[m]];
        q.minl[m] = level[m] - 1; q.maxl[m] = level[m];
    }
    return q;
}

WinQueries window_queries_frame(int n_last, const uint8_t* valid, const int32_t* last_octave, const float* scale_factors, float th)
{
    WinQueries q{ std::vector<float>(n_last), std::vector<int32_t>(n_last), std::vector<int32_t>(n_last) };
    for (int i = 0; i < n_last; i++) {
        if (!valid[i]) { q.qr[i] = -1.f; q.minl[i] = 0; q.maxl[i] = 0; continue; }
        q.qr[i] = th * scale_factors[last_octave[i]];                         // :1401
        q.minl[i] = last_octave[i] - 1; q.maxl[i] = last_octave[i] + 1;       // :1405
    }
    return q;
}

int window_accept_projection_host(int n_mp, const uint8_t* in_view, const int32_t* ci, const int32_t* cd, const int32_t* cn, int cap,
                                  const int32_t* kp_octave, const uint8_t* mp_has_obs, uint8_t* occupied, float nnratio, int32_t* match)
{
    int nmatches = 0;
    for (int m = 0; m < n_mp; m++) {
        if (!in_view[m] || cn[m] == 0) continue;
        int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
        for (int k = 0; k < cn[m]; k++) {
            const int idx = ci[(size_t)m * cap + k];
            if (occupied[idx]) continue;                                       // mvpMapPoints[idx] with Observations() > 0
            const int dist = cd[(size_t)m * cap + k];
            if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = kp_octave[idx]; bestIdx = idx; }
            else if (dist < bestDist2) { bestLevel2 = kp_octave[idx]; bestDist2 = dist; }
        }
        if (bestDist <= 100) {                                                 // TH_HIGH
            if (bestLevel == bestLevel2 && bestDist > nnratio * bestDist2) continue;
            match[bestIdx] = m;
            occupied[bestIdx] = mp_has_obs[m];
            nmatches++;
        }
    }
    return nmatches;
}

int window_accept_frame_host(int n_last, const uint8_t* valid, const int32_t* ci, const int32_t* cd, const int32_t* cn, int cap,
                             const uint8_t* mp_has_obs, uint8_t* occupied, int orb_dist, int check_ori, const float* last_angle,
                             const float* cur_angle, int32_t* match)
{
    RotHisto rot;
    int nmatches = 0;
    for (int i = 0; i < n_last; i++) {
        if (!valid[i] || cn[i] == 0) continue;
        int bestDist = 256, bestIdx2 = -1;
        for (int k = 0; k < cn[i]; k++) {
            const int i2 = ci[(size_t)i * cap + k];
            if (occupied[i2]) continue;
            const int dist = cd[(size_t)i * cap + k];
            if (dist < bestDist) { bestDist = dist; bestIdx2 = i2; }
        }
        if (bestDist <= orb_dist) {                                            // TH_HIGH (:1432) / ORBdist (:1556)
            match[bestIdx2] = i;
            occupied[bestIdx2] = mp_has_obs[i];
            nmatches++;
            if (check_ori) rot.add(last_angle[i] - cur_angle[bestIdx2], bestIdx2);
        }
    }
    if (check_ori) for (int idx : rot.outliers()) { match[idx] = -1; nmatches--; }
    return nmatches;
}

int window_accept_sim3_host(int n_mp, const uint8_t* valid, const int32_t* level, const int32_t* ci, const int32_t* cd, const int32_t* cn, int cap,
                            const int32_t* kp_octave, const uint8_t* observed, uint8_t* matched, int32_t* best_idx, int32_t* best_dist)
{
    int nmatches = 0;
    for (int m = 0; m < n_mp; m++) {                           // sequential: vpMatched grows while the points are visited
        if (best_dist) best_dist[m] = 256;
        if (!valid[m]) continue;
        const int lvl = level[m];
        int bestDist = 256, bestIdx = -1;
        for (int k = 0; k < cn[m]; k++) {
            const int idx = ci[(size_t)m * cap + k];
            if (matched[idx]) continue;                                                              // :393-394
            const int kpLevel = kp_octave[idx];
            if (kpLevel < lvl - 1 || kpLevel > lvl) continue;
            const int dist = cd[(size_t)m * cap + k];
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
        }
        if (bestDist <= 50) {                                                                        // TH_LOW
            best_idx[m] = bestIdx;
            if (best_dist) best_dist[m] = bestDist;
            if (!observed[m]) { matched[bestIdx] = 1; nmatches++; }                                  // :436-440
        }
    }
    return nmatches;
}

extern "C" {

int ccm_window_candidates(ccm_ctx* c, const ccm_frame_grid* f, int nq, const float* qx, const float* qy, const float* qr,
                          const int32_t* min_level, const int32_t* max_level, const uint8_t* qdesc, int cap,
                          int32_t* cand_idx, int32_t* cand_dist, int32_t* cand_n)
{
    return ccm_guard(c, "ccm_window_candidates", [&]() -> int {
        if (!c || !f) return CCM_E_ARG;
        if (nq == 0) return CCM_OK;
        if (nq < 0 || cap < 1 || f->n < 0 || f->grid_cols < 1 || f->grid_rows < 1 || !qx || !qy || !qr || !min_level || !max_level || !qdesc ||
            !cand_idx || !cand_dist || !cand_n || (f->n > 0 && (!f->kp_x || !f->kp_y || !f->kp_octave || !f->desc)))
            return ccm_fail(c, CCM_E_ARG, "bad window-search arguments");
        CCM_HIP(c, hipSetDevice(c->device));
        WinLists L;
        int rc = window_stage(c, f, nq, qx, qy, qr, min_level, max_level, qdesc, L);
        if (rc || (rc = window_lists_launch(c, L, cap)) || (rc = window_lists_fetch(c, L, cap, cand_idx, cand_dist, cand_n))) return rc;   // truncated lists too
        for (int q = 0; q < nq; q++) if (cand_n[q] > cap) return ccm_fail(c, CCM_E_CAPACITY, "query %d has %d candidates, cap %d", q, cand_n[q], cap);
        return CCM_OK;
    });
}

// ORBmatcher::SearchByProjection(Frame&, const vector<mpptr>&, th), ORBmatcher.cpp:71-148
int ccm_search_by_projection(ccm_ctx* c, const ccm_frame_grid* f, const float* scale_factors, int n_mp, const uint8_t* in_view,
                             const int32_t* level, const float* view_cos, const float* proj_x, const float* proj_y,
                             const uint8_t* mp_desc, const uint8_t* mp_has_obs, uint8_t* occupied, float th, float nnratio,
                             int32_t* match)
{
    return ccm_guard(c, "ccm_search_by_projection", [&]() -> int {
        if (!c || !f) return CCM_E_ARG;
        if (f->n < 0 || n_mp < 0 || (f->n > 0 && (!match || !occupied)) ||
            (n_mp > 0 && (!scale_factors || !in_view || !level || !view_cos || !proj_x || !proj_y || !mp_desc || !mp_has_obs)))
            return ccm_fail(c, CCM_E_ARG, "bad SearchByProjection arguments");
        for (int i = 0; i < f->n; i++) match[i] = -1;
        if (n_mp == 0 || f->n == 0) return 0;
        CCM_HIP(c, hipSetDevice(c->device));
        const WinQueries q = window_queries_projection(n_mp, in_view, level, view_cos, scale_factors, th);
        WinLists L;
        int rc = window_stage(c, f, n_mp, proj_x, proj_y, q.qr.data(), q.minl.data(), q.maxl.data(), mp_desc, L);
        if (rc) return rc;
        if (!window_host_accept_forced() && match_window_greedy_lds(f->n, n_mp) <= kGreedyLdsMax)
            return window_greedy(c, L, 0, in_view, nullptr, mp_has_obs, occupied, f->n, nnratio, match, f->n);
        WinHostLists H{ 64 };
        if ((rc = window_lists_host(c, L, H))) return rc;
        return window_accept_projection_host(n_mp, in_view, H.ci.data(), H.cd.data(), H.cn.data(), H.cap, f->kp_octave, mp_has_obs, occupied, nnratio, match);
    });
}

// ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th), ORBmatcher.cpp:1350-1476
int ccm_search_by_projection_frame(ccm_ctx* c, const ccm_frame_grid* f, const float* cur_angle, const float* scale_factors, int n_last,
                                   const uint8_t* valid, const float* u, const float* v, const int32_t* last_octave, const float* last_angle,
                                   const uint8_t* mp_desc, const uint8_t* mp_has_obs, uint8_t* occupied, float th, int check_ori,
                                   int orb_dist, int32_t* match)
{
    return ccm_guard(c, "ccm_search_by_projection_frame", [&]() -> int {
        if (!c || !f) return CCM_E_ARG;
        if (f->n < 0 || n_last < 0 || (f->n > 0 && (!match || !occupied || (check_ori && !cur_angle))) ||
            (n_last > 0 && (!scale_factors || !valid || !u || !v || !last_octave || !mp_desc || !mp_has_obs || (check_ori && !last_angle))))
            return ccm_fail(c, CCM_E_ARG, "bad SearchByProjection(frame, frame) arguments");
        for (int i = 0; i < f->n; i++) match[i] = -1;
        if (n_last == 0 || f->n == 0) return 0;
        CCM_HIP(c, hipSetDevice(c->device));
        const WinQueries q = window_queries_frame(n_last, valid, last_octave, scale_factors, th);
        WinLists L;
        int rc = window_stage(c, f, n_last, u, v, q.qr.data(), q.minl.data(), q.maxl.data(), mp_desc, L);
        if (rc) return rc;
        if (!window_host_accept_forced() && match_window_greedy_lds(f->n, n_last) <= kGreedyLdsMax)
            return window_greedy(c, L, 2, valid, nullptr, mp_has_obs, occupied, f->n, 0.f, match, f->n, orb_dist, check_ori, last_angle, cur_angle);
        WinHostLists H{ 64 };
        if ((rc = window_lists_host(c, L, H))) return rc;
        return window_accept_frame_host(n_last, valid, H.ci.data(), H.cd.data(), H.cn.data(), H.cap, mp_has_obs, occupied, orb_dist, check_ori, last_angle,
                                        cur_angle, match);
    });
}

// ORBmatcher::SearchForInitialization, ORBmatcher.cpp:448-563
int ccm_search_for_initialization(ccm_ctx* c, int n1, const int32_t* oct1, const uint8_t* desc1, const float* angle1,
                                  const ccm_frame_grid* f2, const float* angle2, float* prev_matched_xy, int window, float nnratio,
                                  int check_ori, int32_t* matches12)
{
    return ccm_guard(c, "ccm_search_for_initialization", [&]() -> int {
        if (!c || !f2) return CCM_E_ARG;
        if (n1 < 0 || f2->n < 0 || (n1 > 0 && (!oct1 || !desc1 || !prev_matched_xy || !matches12 || (check_ori && !angle1))) ||
            (check_ori && f2->n > 0 && !angle2))
            return ccm_fail(c, CCM_E_ARG, "bad SearchForInitialization arguments");
        for (int i = 0; i < n1; i++) matches12[i] = -1;
        if (n1 == 0 || f2->n == 0) return 0;
        CCM_HIP(c, hipSetDevice(c->device));
        std::vector<float> qx(n1), qy(n1), qr(n1); std::vector<int32_t> minl(n1), maxl(n1);
        for (int i = 0; i < n1; i++) {
            qx[i] = prev_matched_xy[2 * i]; qy[i] = prev_matched_xy[2 * i + 1];
            qr[i] = oct1[i] > 0 ? -1.f : (float)window;                             // :464-466 only level-0 features
            minl[i] = oct1[i]; maxl[i] = oct1[i];
        }
        WinLists L;
        WinHostLists H{ 128 };
        int rc = window_stage(c, f2, n1, qx.data(), qy.data(), qr.data(), minl.data(), maxl.data(), desc1, L);
        if (rc || (rc = window_lists_host(c, L, H))) return rc;
        RotHisto rot;
        std::vector<int> matched_dist(f2->n, INT32_MAX), m21(f2->n, -1);
        int nmatches = 0;
        for (int i1 = 0; i1 < n1; i1++) {
            if (oct1[i1] > 0 || H.cn[i1] == 0) continue;
            int bestDist = INT32_MAX, bestDist2 = INT32_MAX, bestIdx2 = -1;
            for (int k = 0; k < H.cn[i1]; k++) {
                const int i2 = H.ci[(size_t)i1 * H.cap + k], dist = H.cd[(size_t)i1 * H.cap + k];
                if (matched_dist[i2] <= dist) continue;
                if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx2 = i2; }
                else if (dist < bestDist2) bestDist2 = dist;
            }
            if (bestDist <= 50) {                                                   // TH_LOW
                if (bestDist < (float)bestDist2 * nnratio) {
                    if (m21[bestIdx2] >= 0) { matches12[m21[bestIdx2]] = -1; nmatches--; }
                    matches12[i1] = bestIdx2; m21[bestIdx2] = i1; matched_dist[bestIdx2] = bestDist;
                    nmatches++;
                    if (check_ori) rot.add(angle1[i1] - angle2[bestIdx2], i1);
                }
            }
        }
        if (check_ori)
            for (int idx1 : rot.outliers()) if (matches12[idx1] >= 0) { matches12[idx1] = -1; nmatches--; }
        for (int i1 = 0; i1 < n1; i1++)
            if (matches12[i1] >= 0) { prev_matched_xy[2 * i1] = f2->kp_x[matches12[i1]]; prev_matched_xy[2 * i1 + 1] = f2->kp_y[matches12[i1]]; }
        return nmatches;
    });
}

// Selection loop of ORBmatcher::Fuse, both overloads (ORBmatcher.cpp:914-955 and :1072-1100)
int ccm_fuse_select(ccm_ctx* c, const ccm_frame_grid* kf, const float* scale_factors, const float* inv_level_sigma2, int n_mp,
                    const uint8_t* valid, const float* u, const float* v, const int32_t* level, const uint8_t* mp_desc, float th,
                    int chi2_check, int accept_th, int32_t* best_idx, int32_t* best_dist)
{
    return ccm_guard(c, "ccm_fuse_select", [&]() -> int {
        if (!c || !kf) return CCM_E_ARG;
        if (n_mp < 0 || kf->n < 0 || (n_mp > 0 && (!valid || !u || !v || !level || !mp_desc || !best_idx || !best_dist || !scale_factors)) ||
            (chi2_check && !inv_level_sigma2))
            return ccm_fail(c, CCM_E_ARG, "bad Fuse arguments");
        for (int m = 0; m < n_mp; m++) { best_idx[m] = -1; best_dist[m] = 256; }
        if (n_mp == 0 || kf->n == 0) return CCM_OK;
        CCM_HIP(c, hipSetDevice(c->device));
        std::vector<float> qr(n_mp); std::vector<int32_t> lo(n_mp), hi(n_mp);
        int n_levels = 1;
        for (int m = 0; m < n_mp; m++) {
            qr[m] = valid[m] ? th * scale_factors[level[m]] : -1.f;                                  // :909 / :1068
            lo[m] = level[m] - 1; hi[m] = level[m];                                                  // :925-926 kpLevel in [level - 1, level]
        }
        for (int i = 0; i < kf->n; i++) n_levels = std::max(n_levels, kf->kp_octave[i] + 1);
        // the whole selection runs on the device (k_window_select): one (index, distance) per map point comes back, no candidate list
        WindowBufs& W = window_bufs(c);
        WinLists L;
        int rc = window_stage(c, kf, n_mp, u, v, qr.data(), lo.data(), hi.data(), mp_desc, L);
        if (rc || (chi2_check && (rc = ccm_upload(c, W.is2, inv_level_sigma2, (size_t)n_levels * 4, c->stream)))) return rc;
        CCM_RESERVE(c, W.sel_i, (size_t)n_mp * 4); CCM_RESERVE(c, W.sel_d, (size_t)n_mp * 4);
        match_launch_window_select(c->stream, L.grid, n_mp, L.qx, L.qy, L.qr, L.minl, L.maxl, L.qdesc, chi2_check ? W.is2.as<float>() : nullptr, accept_th,
                                   W.sel_i.as<int>(), W.sel_d.as<int>());
        CCM_HIP(c, hipGetLastError());
        CCM_HIP(c, hipMemcpyAsync(best_idx, W.sel_i.p, (size_t)n_mp * 4, hipMemcpyDeviceToHost, c->stream));
        CCM_HIP(c, hipMemcpyAsync(best_dist, W.sel_d.p, (size_t)n_mp * 4, hipMemcpyDeviceToHost, c->stream));
        CCM_HIP(c, hipStreamSynchronize(c->stream));
        for (int m = 0; m < n_mp; m++) if (!valid[m]) { best_idx[m] = -1; best_dist[m] = 256; }
        return CCM_OK;
    });
}

// What ccm_fuse_select_batch and ccm_fuse_select_batch_frames share once the WinGrid table lies in W.grids: the per-query windows,
// the uploads of the queries, the launch, the download and the rows of invalid points and empty keyframes.  kf_n[k] = features of
// keyframe k; n_levels = entries of inv_level_sigma2 the kernel may read.
static int fuse_batch_run(ccm_ctx* c, int n_kf, const int* kf_n, int n_levels, const float* scale_factors, const float* inv_level_sigma2,
                          const int32_t* mp_first, const uint8_t* valid, const float* u, const float* v, const int32_t* level,
                          const uint8_t* mp_desc, float th, int chi2_check, int accept_th, int32_t* best_idx, int32_t* best_dist)
{
    WindowBufs& W = window_bufs(c);
    const int n_mp = mp_first[n_kf];
    std::vector<float> qr(n_mp);
    std::vector<int32_t> lo(n_mp), hi(n_mp), qkf(n_mp);
    for (int k = 0; k < n_kf; k++)
        for (int m = mp_first[k]; m < mp_first[k + 1]; m++) {
            qkf[m] = k;
            qr[m] = (valid[m] && kf_n[k] > 0) ? th * scale_factors[level[m]] : -1.f;                  // :909 / :1068
            lo[m] = level[m] - 1; hi[m] = level[m];                                               // :925-926
        }
    hipStream_t st = c->stream;
    WinLists L;
    int rc = window_stage_queries(c, WinGrid{}, n_mp, u, v, qr.data(), lo.data(), hi.data(), mp_desc, qkf.data(), L);
    if (rc || (chi2_check && (rc = ccm_upload(c, W.is2, inv_level_sigma2, (size_t)n_levels * 4, st)))) return rc;
    CCM_RESERVE(c, W.sel_i, (size_t)n_mp * 4); CCM_RESERVE(c, W.sel_d, (size_t)n_mp * 4);
    match_launch_window_select_batch(st, L.grids, L.q_kf, n_mp, L.qx, L.qy, L.qr, L.minl, L.maxl, L.qdesc, chi2_check ? W.is2.as<float>() : nullptr, accept_th,
                                     W.sel_i.as<int>(), W.sel_d.as<int>());
    CCM_HIP(c, hipGetLastError());
    CCM_HIP(c, hipMemcpyAsync(best_idx, W.sel_i.p, (size_t)n_mp * 4, hipMemcpyDeviceToHost, st));
    CCM_HIP(c, hipMemcpyAsync(best_dist, W.sel_d.p, (size_t)n_mp * 4, hipMemcpyDeviceToHost, st));
    CCM_HIP(c, hipStreamSynchronize(st));                           // (the staging vectors above, and the caller's, stay alive until here)
    for (int m = 0; m < n_mp; m++) if (!valid[m] || kf_n[qkf[m]] == 0) { best_idx[m] = -1; best_dist[m] = 256; }
    return CCM_OK;
}

// The argument checks the two batch entry points open with (kfs: either kind of keyframe array, only tested for null)
static int fuse_batch_check(ccm_ctx* c, int n_kf, const void* kfs, const float* scale_factors, const float* inv_level_sigma2, const int32_t* mp_first,
                            const uint8_t* valid, const float* u, const float* v, const int32_t* level, const uint8_t* mp_desc, int chi2_check,
                            const int32_t* best_idx, const int32_t* best_dist)
{
    if (!c) return CCM_E_ARG;
    if (n_kf < 0 || (n_kf > 0 && (!kfs || !mp_first))) return ccm_fail(c, CCM_E_ARG, "bad Fuse batch arguments");
    if (n_kf == 0) return CCM_OK;
    const int n_mp = mp_first[n_kf];
    if (mp_first[0] != 0 || n_mp < 0 || (n_mp > 0 && (!valid || !u || !v || !level || !mp_desc || !best_idx || !best_dist || !scale_factors)) ||
        (chi2_check && !inv_level_sigma2))
        return ccm_fail(c, CCM_E_ARG, "bad Fuse batch arguments");
    return CCM_OK;
}

// The selection of ccm_fuse_select for n_kf keyframes in one launch: what n_kf sequential calls return (the selection reads the map
// points' projections and descriptors and the keyframe's features only -- what an earlier keyframe's Replace / AddObservation
// changes is which points the CALLER still applies, src/ORBmatcher.cpp:884-886, :958-990).  Map points projected into keyframe k are
// rows mp_first[k] .. mp_first[k + 1] - 1 of valid / u / v / level / mp_desc and of the outputs.
int ccm_fuse_select_batch(ccm_ctx* c, int n_kf, const ccm_frame_grid* kfs, const float* scale_factors, const float* inv_level_sigma2,
                          const int32_t* mp_first, const uint8_t* valid, const float* u, const float* v, const int32_t* level,
                          const uint8_t* mp_desc, float th, int chi2_check, int accept_th, int32_t* best_idx, int32_t* best_dist)
{
    return ccm_guard(c, "ccm_fuse_select_batch", [&]() -> int {
        int rc = fuse_batch_check(c, n_kf, kfs, scale_factors, inv_level_sigma2, mp_first, valid, u, v, level, mp_desc, chi2_check, best_idx, best_dist);
        if (rc || n_kf == 0) return rc;
        const int n_mp = mp_first[n_kf];
        for (int k = 0; k < n_kf; k++)
            if (mp_first[k + 1] < mp_first[k] || kfs[k].n < 0 || kfs[k].grid_cols < 1 || kfs[k].grid_rows < 1)
                return ccm_fail(c, CCM_E_ARG, "bad Fuse batch arguments");
        for (int m = 0; m < n_mp; m++) { best_idx[m] = -1; best_dist[m] = 256; }
        if (n_mp == 0) return CCM_OK;
        CCM_HIP(c, hipSetDevice(c->device));
        KfBatch B;
        if ((rc = stage_keyframes(c, n_kf, kfs, B))) return rc;
        std::vector<int> kf_n(n_kf);
        for (int k = 0; k < n_kf; k++) kf_n[k] = kfs[k].n;
        return fuse_batch_run(c, n_kf, kf_n.data(), B.n_levels, scale_factors, inv_level_sigma2, mp_first, valid, u, v, level, mp_desc, th, chi2_check,
                              accept_th, best_idx, best_dist);
    });
}

// ccm_fuse_select_batch on frame handles: the WinGrid table is built from the handles' device pointers and device-built grids
// (stage_keyframes uploads nothing).  Queries and outputs as above.
int ccm_fuse_select_batch_frames(ccm_ctx* c, int n_kf, ccm_frame* const* kfs, const float* scale_factors, const float* inv_level_sigma2,
                                 const int32_t* mp_first, const uint8_t* valid, const float* u, const float* v, const int32_t* level,
                                 const uint8_t* mp_desc, float th, int chi2_check, int accept_th, int32_t* best_idx, int32_t* best_dist)
{
    return ccm_guard(c, "ccm_fuse_select_batch_frames", [&]() -> int {
        int rc = fuse_batch_check(c, n_kf, kfs, scale_factors, inv_level_sigma2, mp_first, valid, u, v, level, mp_desc, chi2_check, best_idx, best_dist);
        if (rc || n_kf == 0) return rc;
        const int n_mp = mp_first[n_kf];
        int n_levels = 1;
        for (int k = 0; k < n_kf; k++) {
            if (mp_first[k + 1] < mp_first[k] || !kfs[k]) return ccm_fail(c, CCM_E_ARG, "bad Fuse batch arguments");
            if ((rc = frame_check(c, kfs[k]))) return rc;
            n_levels = std::max(n_levels, kfs[k]->n_levels);
        }
        for (int m = 0; m < n_mp; m++) { best_idx[m] = -1; best_dist[m] = 256; }
        if (n_mp == 0) return CCM_OK;
        CCM_HIP(c, hipSetDevice(c->device));
        std::vector<WinGrid> grids(n_kf);
        std::vector<int> kf_n(n_kf);
        for (int k = 0; k < n_kf; k++) {
            const ccm_frame* f = kfs[k];
            grids[k] = frame_win_grid(f);
            kf_n[k] = f->n;
        }
        if ((rc = ccm_upload(c, window_bufs(c).grids, grids.data(), grids.size() * sizeof(WinGrid), c->stream))) return rc;
        return fuse_batch_run(c, n_kf, kf_n.data(), n_levels, scale_factors, inv_level_sigma2, mp_first, valid, u, v, level, mp_desc, th, chi2_check,
                              accept_th, best_idx, best_dist);
    });
}

// ORBmatcher::SearchBySim3, ORBmatcher.cpp:1124-1348: two selection passes (<= TH_HIGH) and the agreement check
int ccm_search_by_sim3(ccm_ctx* c, const ccm_frame_grid* kf1, const float* scale_factors1, const ccm_frame_grid* kf2, const float* scale_factors2,
                       const uint8_t* valid1, const float* u1, const float* v1, const int32_t* level1, const uint8_t* mp_desc1,
                       const uint8_t* valid2, const float* u2, const float* v2, const int32_t* level2, const uint8_t* mp_desc2,
                       float th, int32_t* match12)
{
    return ccm_guard(c, "ccm_search_by_sim3", [&]() -> int {
        if (!c || !kf1 || !kf2) return CCM_E_ARG;
        if (kf1->n < 0 || kf2->n < 0 || (kf1->n > 0 && !match12)) return ccm_fail(c, CCM_E_ARG, "bad SearchBySim3 arguments");
        const int n1 = kf1->n, n2 = kf2->n;
        std::vector<int32_t> m1(std::max(n1, 1)), d1(std::max(n1, 1)), m2(std::max(n2, 1)), d2(std::max(n2, 1));
        // map points of KF1 (one per feature of KF1) are searched in KF2, and vice versa
        int rc = ccm_fuse_select(c, kf2, scale_factors2, nullptr, n1, valid1, u1, v1, level1, mp_desc1, th, 0, 100, m1.data(), d1.data());
        if (rc) return rc;
        rc = ccm_fuse_select(c, kf1, scale_factors1, nullptr, n2, valid2, u2, v2, level2, mp_desc2, th, 0, 100, m2.data(), d2.data());
        if (rc) return rc;
        int nFound = 0;
        for (int i1 = 0; i1 < n1; i1++) {
            match12[i1] = -1;
            const int idx2 = m1[i1];
            if (idx2 >= 0 && m2[idx2] == i1) { match12[i1] = idx2; nFound++; }     // :1330-1345
        }
        return nFound;
    });
}

// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th), ORBmatcher.cpp:308-446
int ccm_search_by_projection_sim3(ccm_ctx* c, const ccm_frame_grid* kf, const float* scale_factors, int n_mp, const uint8_t* valid,
                                  const float* u, const float* v, const int32_t* level, const uint8_t* mp_desc, const uint8_t* observed,
                                  uint8_t* matched, float th, int32_t* best_idx)
{
    return ccm_guard(c, "ccm_search_by_projection_sim3", [&]() -> int {
        if (!c || !kf) return CCM_E_ARG;
        if (n_mp < 0 || kf->n < 0 || (n_mp > 0 && (!valid || !u || !v || !level || !mp_desc || !observed || !best_idx || !scale_factors)) ||
            (kf->n > 0 && !matched))
            return ccm_fail(c, CCM_E_ARG, "bad SearchByProjection(kf, Scw) arguments");
        for (int m = 0; m < n_mp; m++) best_idx[m] = -1;
        if (n_mp == 0 || kf->n == 0) return 0;
        CCM_HIP(c, hipSetDevice(c->device));
        std::vector<float> qr(n_mp); std::vector<int32_t> none(n_mp, -1);
        for (int m = 0; m < n_mp; m++) qr[m] = valid[m] ? th * scale_factors[level[m]] : -1.f;       // :380
        WinLists L;
        int rc = window_stage(c, kf, n_mp, u, v, qr.data(), none.data(), none.data(), mp_desc, L);
        if (rc) return rc;
        if (!window_host_accept_forced() && match_window_greedy_lds(kf->n, n_mp) <= kGreedyLdsMax)
            return window_greedy(c, L, 1, valid, level, observed, matched, kf->n, 0.f, best_idx, n_mp);
        WinHostLists H{ 64 };
        if ((rc = window_lists_host(c, L, H))) return rc;
        return window_accept_sim3_host(n_mp, valid, level, H.ci.data(), H.cd.data(), H.cn.data(), H.cap, kf->kp_octave, observed, matched, best_idx);
    });
}

// ccm_search_by_projection_sim3 for n_kf keyframes in ONE launch of each kernel (the loop closer matches the loop points into every
// keyframe connected to the current one, src/LoopFinder.cpp / MapMatcher.cpp: one SearchByProjection(pKF, Scw, ...) per keyframe).
// Keyframes are independent problems -- each has its own vpMatched -- so workgroup k of k_window_greedy takes keyframe k.
int ccm_search_by_projection_sim3_batch(ccm_ctx* c, int n_kf, const ccm_frame_grid* kfs, const float* scale_factors, const int32_t* mp_first,
                                        const uint8_t* valid, const float* u, const float* v, const int32_t* level, const uint8_t* mp_desc,
                                        const uint8_t* observed, uint8_t* matched, float th, int32_t* best_idx, int32_t* n_matches)
{
    return ccm_guard(c, "ccm_search_by_projection_sim3_batch", [&]() -> int {
        if (!c) return CCM_E_ARG;
        if (n_kf < 0 || (n_kf > 0 && (!kfs || !mp_first || !n_matches))) return ccm_fail(c, CCM_E_ARG, "bad SearchByProjection(kf, Scw) batch arguments");
        if (n_kf == 0) return 0;
        const int n_mp = mp_first[n_kf];
        if (mp_first[0] != 0 || n_mp < 0 || (n_mp > 0 && (!valid || !u || !v || !level || !mp_desc || !observed || !best_idx || !scale_factors)))
            return ccm_fail(c, CCM_E_ARG, "bad SearchByProjection(kf, Scw) batch arguments");
        int max_n = 0, NF = 0;
        for (int k = 0; k < n_kf; k++) {
            if (mp_first[k + 1] < mp_first[k] || kfs[k].n < 0 || kfs[k].grid_cols < 1 || kfs[k].grid_rows < 1)
                return ccm_fail(c, CCM_E_ARG, "bad SearchByProjection(kf, Scw) batch arguments");
            NF += kfs[k].n;
            max_n = std::max(max_n, kfs[k].n);
            n_matches[k] = 0;
        }
        if (NF > 0 && !matched) return ccm_fail(c, CCM_E_ARG, "bad SearchByProjection(kf, Scw) batch arguments");
        for (int m = 0; m < n_mp; m++) best_idx[m] = -1;
        if (n_mp == 0 || NF == 0) return 0;
        if (window_host_accept_forced() || match_window_greedy_lds(max_n, 0) > kGreedyLdsMax) {          // keyframe by keyframe through the single entry point
            int total = 0;
            for (int k = 0, f0 = 0; k < n_kf; f0 += kfs[k].n, k++) {
                const int q0 = mp_first[k], nq = mp_first[k + 1] - q0;
                const int r = ccm_search_by_projection_sim3(c, &kfs[k], scale_factors, nq, valid + q0, u + q0, v + q0, level + q0, mp_desc + (size_t)q0 * 32,
                                                            observed + q0, matched + f0, th, best_idx + q0);
                if (r < 0) return r;
                n_matches[k] = r; total += r;
            }
            return total;
        }
        CCM_HIP(c, hipSetDevice(c->device));
        KfBatch B;
        int rc = stage_keyframes(c, n_kf, kfs, B);
        if (rc) return rc;
        std::vector<float> qr(n_mp);
        std::vector<int32_t> none(n_mp, -1), qkf(n_mp);
        std::vector<GreedyKf> gk(n_kf);
        for (int k = 0; k < n_kf; k++) {
            for (int m = mp_first[k]; m < mp_first[k + 1]; m++) {
                qkf[m] = k;
                qr[m] = (valid[m] && kfs[k].n > 0) ? th * scale_factors[level[m]] : -1.f;              // :380
            }
            gk[k] = GreedyKf{ mp_first[k], mp_first[k + 1] - mp_first[k], B.feat_first[k], kfs[k].n };
        }
        WinLists L;
        if ((rc = window_stage_queries(c, WinGrid{}, n_mp, u, v, qr.data(), none.data(), none.data(), mp_desc, qkf.data(), L))) return rc;
        return window_greedy(c, L, 1, valid, level, observed, matched, NF, 0.f, best_idx, n_mp, 0, 0, nullptr, nullptr, &gk, max_n, n_matches);
    });
}
}  // extern "C"
