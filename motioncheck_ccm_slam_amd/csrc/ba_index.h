// ba_index.h -- host-side index of a bundle adjustment's edge list: this rank's edges in (landmark, keyframe) order and the two
// CSR structures the kernels walk (landmark -> edges, free keyframe -> edges).  Host only, standard library only: ba_host.cpp uses
// it, tests/support/ba_index_check.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

// The result owns its staging copies: the pointers e_pose .. e_info stay valid as long as it lives (and as long as the caller's
// arrays do, when `direct`).  Movable, not copyable.
struct BaEdgeIndex {
    long long out_of_range = -1;           // lowest edge with a vertex index out of range; nothing else is filled in then
    bool direct = false;                   // the caller's list is sorted and wholly this rank's: used where it lies
    int E = 0;                             // this rank's edges
    std::vector<int> perm;                 // [E] position -> the caller's edge id (empty when direct)
    const int32_t* e_pose = nullptr;       // [E] keyframe of the edge at a position
    const int32_t* e_pt = nullptr;         // [E] landmark, counted from the shard's first (l0)
    const double* e_obs = nullptr;         // [E][2]
    const double* e_info = nullptr;        // [E]
    std::vector<int> pt_first;             // [L+1] CSR landmark -> positions
    std::vector<int> pose_first;           // [nfree+1] CSR free keyframe -> pose_edges
    std::unique_ptr<int[]> pose_edges;     // [n_pose_edges] positions, ascending per keyframe (every slot is written: no zero-fill of 7 MB)
    size_t n_pose_edges = 0;

    BaEdgeIndex() = default;
    BaEdgeIndex(BaEdgeIndex&&) = default;
    BaEdgeIndex& operator=(BaEdgeIndex&&) = default;

    // a list something else has checked and indexed (the device path): the caller's arrays, no host index
    static BaEdgeIndex unindexed(const int32_t* edge_pose, const int32_t* edge_point, const double* obs, const double* info, int n_edges)
    {
        BaEdgeIndex ix;
        ix.direct = true; ix.E = n_edges;
        ix.e_pose = edge_pose; ix.e_pt = edge_point; ix.e_obs = obs; ix.e_info = info;
        return ix;
    }

    // position -> the caller's edge id
    int edge_id(int k) const { return direct ? k : perm[k]; }

    // staging copies behind e_pose .. e_info (empty when direct)
    std::vector<int> e_pose_v, e_pt_v;
    std::vector<double> e_obs_v, e_info_v;
};

// Runs fn(0) .. fn(nt-1), on nt threads where the system gives them (contiguous slices; every result is the same as the serial loop's).
template <class F> inline void ba_index_pfor(int nt, F&& fn)
{
    if (nt == 1) { fn(0); return; }
    std::vector<std::thread> th;
    int started = 1;                                   // slices 1 .. started-1 have a thread
    try { for (int t = 1; t < nt; t++) { th.emplace_back([&fn, t]() { fn(t); }); started = t + 1; } }
    catch (const std::system_error&) {}                // thread or process limit: the remaining slices run here, same results
    fn(0);
    for (int t = started; t < nt; t++) fn(t);
    for (auto& x : th) x.join();
}
inline std::pair<long long, long long> ba_index_slice(long long total, int t, int nt) { return { total * t / nt, total * (t + 1) / nt }; }

// Indexes the edges whose landmark lies in [l0, l1) of a list of n_edges edges over n_poses keyframes and n_points landmarks.
// free_of[p] = free index of keyframe p or -1 (n_free of them are free).  The passes over the list are dealt to n_threads threads.
//
// local edges sorted by (landmark, pose); perm[k] = original edge id
// (a comparison sort of the 1.8 M edges of config 5 took 20 ms, a fifth of the whole call: a graph extracted landmark by landmark
// arrives sorted already, which one pass detects; otherwise a stable counting sort by landmark and an insertion sort of each
// landmark's handful of observations by keyframe give the same order in linear time)
// The passes over the edge list below were 4 ms of host time at config 5 (1.8 M edges): large graphs deal them to a few threads.
inline BaEdgeIndex ba_index_edges(const int32_t* edge_pose, const int32_t* edge_point, const double* obs, const double* info, int n_edges,
                                  int n_poses, int n_points, int l0, int l1, const int* free_of, int n_free, int n_threads)
{
    BaEdgeIndex ix;
    const int NT = std::max(1, n_threads), Eall = n_edges, L = l1 - l0, nfree = n_free;
    bool sorted = true;
    int n_local = 0;
    {
        std::vector<int> cnt(NT, 0), bad(NT, 0), first_l(NT, -1), first_p(NT, -1), last_l(NT, -1), last_p(NT, -1);
        std::vector<long long> out_of_range(NT, -1);
        ba_index_pfor(NT, [&](int t) {
            const auto r = ba_index_slice(Eall, t, NT);
            int prev_l = -1, prev_p = -1, c = 0, b = 0;
            for (long long e = r.first; e < r.second; e++) {
                const int l = edge_point[e];
                const int p = edge_pose[e];
                if (p < 0 || p >= n_poses || l < 0 || l >= n_points) { if (out_of_range[t] < 0) out_of_range[t] = e; continue; }
                if (l < l0 || l >= l1) continue;
                if (c == 0) { first_l[t] = l; first_p[t] = p; }
                else if (l < prev_l || (l == prev_l && p < prev_p)) b = 1;
                prev_l = l; prev_p = p; c++;
            }
            cnt[t] = c; bad[t] = b; last_l[t] = prev_l; last_p[t] = prev_p;
        });
        for (int t = 0; t < NT; t++)
            if (out_of_range[t] >= 0) { ix.out_of_range = out_of_range[t]; return ix; }      // slices ascend: the lowest offending edge
        int pl = -1, pp = -1;
        for (int t = 0; t < NT; t++) {
            if (bad[t]) sorted = false;
            if (cnt[t]) {
                if (first_l[t] < pl || (first_l[t] == pl && first_p[t] < pp)) sorted = false;      // across the slice boundary
                pl = last_l[t]; pp = last_p[t];
            }
            n_local += cnt[t];
        }
    }
    // a sorted, unsharded edge list is used where it lies (no index vector, no staging copies: 6 ms at config 5)
    const bool direct = sorted && n_local == Eall && l0 == 0;
    std::vector<int>& perm = ix.perm;
    if (!direct) {
        perm.reserve(n_local);
        for (int e = 0; e < Eall; e++) { const int l = edge_point[e]; if (l >= l0 && l < l1) perm.push_back(e); }
    }
    if (!sorted) {
        std::vector<int> first(L + 2, 0), out(perm.size());
        for (int e : perm) first[edge_point[e] - l0 + 1]++;
        for (int l = 0; l < L; l++) first[l + 1] += first[l];
        {
            std::vector<int> fill(first.begin(), first.end() - 1);
            for (int e : perm) out[fill[edge_point[e] - l0]++] = e;          // stable: ties keep the input order
        }
        for (int l = 0; l < L; l++)
            for (int a = first[l] + 1; a < first[l + 1]; a++) {                 // stable insertion sort by keyframe
                const int v = out[a], pv = edge_pose[v];
                int b = a - 1;
                while (b >= first[l] && edge_pose[out[b]] > pv) { out[b + 1] = out[b]; b--; }
                out[b + 1] = v;
            }
        perm.swap(out);
    }
    const int E = n_local;
    ix.direct = direct; ix.E = E;
    if (!direct) {
        const bool values = obs && info;       // (the table route has neither on the host: the device gathers them in this order)
        ix.e_pose_v.resize(E); ix.e_pt_v.resize(E);
        if (values) { ix.e_obs_v.resize(2 * (size_t)E); ix.e_info_v.resize(E); }
        for (int k = 0; k < E; k++) {
            const int e = perm[k];
            ix.e_pose_v[k] = edge_pose[e]; ix.e_pt_v[k] = edge_point[e] - l0;
            if (values) { ix.e_obs_v[2 * k] = obs[2 * e]; ix.e_obs_v[2 * k + 1] = obs[2 * e + 1]; ix.e_info_v[k] = info[e]; }
        }
    }
    const int32_t* e_pose = ix.e_pose = direct ? edge_pose : ix.e_pose_v.data();
    const int32_t* e_pt = ix.e_pt = direct ? edge_point : ix.e_pt_v.data();
    ix.e_obs = direct ? obs : ix.e_obs_v.data();
    ix.e_info = direct ? info : ix.e_info_v.data();
    // pt_first: the edges are sorted by landmark, so a landmark's first edge is where the landmark index changes;
    // pose_edges: stable counting sort of the edges by free keyframe, slice by slice
    std::vector<int>& pt_first = ix.pt_first;
    std::vector<int>& pose_first = ix.pose_first;
    pt_first.assign(L + 1, 0);
    pose_first.assign(nfree + 1, 0);
    std::vector<std::vector<int>> hist(NT, std::vector<int>(nfree + 1, 0));
    ba_index_pfor(NT, [&](int t) {
        const auto r = ba_index_slice(E, t, NT);
        std::vector<int>& h = hist[t];
        for (long long k = r.first; k < r.second; k++) {
            const int l = e_pt[k];
            const int lp = k > 0 ? e_pt[k - 1] : -1;
            for (int q = lp + 1; q <= l; q++) pt_first[q] = (int)k;           // landmarks without edges in between start here too
            const int f = free_of[e_pose[k]];
            if (f >= 0) h[f]++;
        }
    });
    const int last = E > 0 ? e_pt[E - 1] : -1;
    for (int q = last + 1; q <= L; q++) pt_first[q] = E;
    // slice t's first slot for keyframe f = all earlier keyframes + f's edges in earlier slices
    int acc = 0;
    for (int f = 0; f < nfree; f++) {
        pose_first[f] = acc;
        for (int t = 0; t < NT; t++) { const int c = hist[t][f]; hist[t][f] = acc; acc += c; }
    }
    pose_first[nfree] = acc;
    ix.n_pose_edges = (size_t)acc; ix.pose_edges.reset(new int[std::max<size_t>(ix.n_pose_edges, 1)]);
    int* pose_edges = ix.pose_edges.get();
    ba_index_pfor(NT, [&](int t) {
        const auto r = ba_index_slice(E, t, NT);
        std::vector<int>& fill = hist[t];
        for (long long k = r.first; k < r.second; k++) { const int f = free_of[e_pose[k]]; if (f >= 0) pose_edges[fill[f]++] = (int)k; }
    });
    return ix;
}
