// TEST SCAFFOLDING: the host edge index of the bundle adjustment (csrc/ba_index.h) against the slow, obvious way -- a
// std::stable_sort of the local edge ids by (landmark, keyframe) and counting loops -- on small edge lists built here.  Integers
// and copied doubles only: every comparison is exact.  Prints one line of key=value pairs; exits 1 at the first mismatch.
//   usage: ba_index_check order | shard | all_fixed | empty | range | threads
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include "../../motioncheck_ccm_slam_amd/csrc/ba_index.h"

struct Edges {
    int P = 0, L = 0;
    std::vector<uint8_t> fixed;
    std::vector<int32_t> pose, pt;
    std::vector<double> obs, info;
    std::vector<int> free_of;
    int nfree = 0;
    int E() const { return (int)pose.size(); }
    void add(int p, int l) { const int e = E(); pose.push_back(p); pt.push_back(l); obs.push_back(e + 0.25); obs.push_back(-e - 0.5); info.push_back(e + 0.125); }
    void finish()
    {
        free_of.assign(P, -1); nfree = 0;
        for (int p = 0; p < P; p++) if (!fixed[p]) free_of[p] = nfree++;
    }
    Edges shuffled(unsigned seed) const
    {
        std::vector<int> o(E());
        std::iota(o.begin(), o.end(), 0);
        std::mt19937 rng(seed);
        std::shuffle(o.begin(), o.end(), rng);
        Edges s = *this;
        for (int k = 0; k < E(); k++) { s.pose[k] = pose[o[k]]; s.pt[k] = pt[o[k]]; s.obs[2 * k] = obs[2 * o[k]]; s.obs[2 * k + 1] = obs[2 * o[k] + 1]; s.info[k] = info[o[k]]; }
        return s;
    }
    BaEdgeIndex index(int l0, int l1, int nt) const
    {
        return ba_index_edges(pose.data(), pt.data(), obs.data(), info.data(), E(), P, L, l0, l1, free_of.data(), nfree, nt);
    }
};

// 7 keyframes of which 0, 3 and 6 are fixed; 12 landmarks of which 0, 5 and 11 have no observation; landmark 7 is seen by the fixed
// keyframes only; (landmark 2, keyframe 4) is there twice.  Sorted by (landmark, keyframe).
static Edges base_case()
{
    Edges g;
    g.P = 7; g.L = 12; g.fixed = {1, 0, 0, 1, 0, 0, 1};
    for (int l = 0; l < g.L; l++) {
        if (l == 0 || l == 5 || l == 11) continue;
        for (int p = 0; p < g.P; p++) {
            const bool seen = l == 7 ? g.fixed[p] != 0 : (l * 3 + p * 5) % 7 < 4 || (l == 2 && p == 4);
            if (!seen) continue;
            g.add(p, l);
            if (l == 2 && p == 4) g.add(p, l);
        }
    }
    g.finish();
    return g;
}

static Edges random_case(int P, int L, int E, unsigned seed)
{
    Edges g;
    g.P = P; g.L = L; g.fixed.assign(P, 0);
    std::mt19937 rng(seed);
    for (int p = 0; p < P; p++) g.fixed[p] = rng() % 5 == 0;
    for (int e = 0; e < E; e++) g.add((int)(rng() % P), (int)(rng() % L));
    g.finish();
    return g;
}

#define REQUIRE(cond) do { if (!(cond)) { printf("FAILED %s: %s (line %d)\n", what, #cond, __LINE__); exit(1); } } while (0)

// every field of ix against the obvious construction; returns the number of local edges
static int check(const char* what, const Edges& g, int l0, int l1, const BaEdgeIndex& ix)
{
    const int L = l1 - l0;
    REQUIRE(ix.out_of_range == -1);
    std::vector<int> ids;
    for (int e = 0; e < g.E(); e++) if (g.pt[e] >= l0 && g.pt[e] < l1) ids.push_back(e);                       // only local edges are kept
    std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) { return g.pt[a] != g.pt[b] ? g.pt[a] < g.pt[b] : g.pose[a] < g.pose[b]; });
    const int E = (int)ids.size();
    REQUIRE(ix.E == E);
    bool identity = E == g.E();
    for (int k = 0; k < E && identity; k++) identity = ids[k] == k;
    REQUIRE(ix.direct == (identity && l0 == 0));
    if (ix.direct) {
        REQUIRE(ix.perm.empty() && ix.e_pose == g.pose.data() && ix.e_pt == g.pt.data() && ix.e_obs == g.obs.data() && ix.e_info == g.info.data());
    } else {
        REQUIRE(ix.perm == ids);
        REQUIRE(E == 0 || (ix.e_pose != g.pose.data() && ix.e_pt != g.pt.data()));
    }
    for (int k = 0; k < E; k++) {
        const int e = ids[k];
        REQUIRE(ix.edge_id(k) == e);
        REQUIRE(ix.e_pose[k] == g.pose[e] && ix.e_pt[k] == g.pt[e] - l0);                                       // landmark indices are rebased
        REQUIRE(ix.e_obs[2 * k] == g.obs[2 * e] && ix.e_obs[2 * k + 1] == g.obs[2 * e + 1] && ix.e_info[k] == g.info[e]);
    }
    REQUIRE((int)ix.pt_first.size() == L + 1);
    std::vector<int> seen(L + 1, 0);
    for (int e : ids) seen[g.pt[e] - l0]++;
    for (int q = 0, below = 0; q <= L; below += seen[q], q++) REQUIRE(ix.pt_first[q] == below);            // local edges with landmark < q
    REQUIRE((int)ix.pose_first.size() == g.nfree + 1 && ix.pose_first[0] == 0);
    for (int f = 0; f < g.nfree; f++) {
        std::vector<int> want;
        for (int k = 0; k < E; k++) if (g.free_of[g.pose[ids[k]]] == f) want.push_back(k);                     // ascending positions
        REQUIRE(ix.pose_first[f + 1] - ix.pose_first[f] == (int)want.size());
        for (size_t i = 0; i < want.size(); i++) REQUIRE(ix.pose_edges[ix.pose_first[f] + i] == want[i]);
    }
    REQUIRE(ix.n_pose_edges == (size_t)ix.pose_first[g.nfree]);
    return E;
}

static void same(const char* what, const BaEdgeIndex& a, const BaEdgeIndex& b)
{
    REQUIRE(a.out_of_range == b.out_of_range && a.direct == b.direct && a.E == b.E && a.perm == b.perm);
    REQUIRE(a.pt_first == b.pt_first && a.pose_first == b.pose_first && a.n_pose_edges == b.n_pose_edges);
    REQUIRE(std::equal(a.pose_edges.get(), a.pose_edges.get() + a.n_pose_edges, b.pose_edges.get()));
    for (int k = 0; k < a.E; k++)
        REQUIRE(a.e_pose[k] == b.e_pose[k] && a.e_pt[k] == b.e_pt[k] && a.e_obs[2 * k] == b.e_obs[2 * k] && a.e_obs[2 * k + 1] == b.e_obs[2 * k + 1] && a.e_info[k] == b.e_info[k]);
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    const Edges g = base_case();
    if (mode == "order") {
        const BaEdgeIndex a = g.index(0, g.L, 1);
        check("sorted", g, 0, g.L, a);
        const Edges s = g.shuffled(7);
        const BaEdgeIndex b = s.index(0, s.L, 1);
        check("shuffled", s, 0, s.L, b);
        printf("edges=%d sorted_direct=%d shuffled_direct=%d\n", g.E(), (int)a.direct, (int)b.direct);
    } else if (mode == "shard") {
        const BaEdgeIndex a = g.index(4, 9, 1);
        const int kept = check("shard of the sorted list", g, 4, 9, a);
        const Edges s = g.shuffled(8);
        const BaEdgeIndex b = s.index(4, 9, 1);
        check("shard of the shuffled list", s, 4, 9, b);
        int lo = 1 << 30, hi = -1;
        for (int k = 0; k < a.E; k++) { lo = std::min(lo, (int)a.e_pt[k]); hi = std::max(hi, (int)a.e_pt[k]); }
        printf("edges=%d kept=%d direct=%d pt_min=%d pt_max=%d\n", g.E(), kept, (int)a.direct, lo, hi);
    } else if (mode == "all_fixed") {
        Edges f = g;
        f.fixed.assign(f.P, 1); f.finish();
        const BaEdgeIndex a = f.index(0, f.L, 1);
        check("all keyframes fixed", f, 0, f.L, a);
        printf("nfree=%d n_pose_edges=%zu pose_first_size=%zu pose_first0=%d\n", f.nfree, a.n_pose_edges, a.pose_first.size(), a.pose_first[0]);
    } else if (mode == "empty") {
        Edges e0 = g;                                          // no edge, 12 landmarks
        e0.pose.clear(); e0.pt.clear(); e0.obs.clear(); e0.info.clear();
        const BaEdgeIndex a = e0.index(0, e0.L, 8);
        check("E = 0", e0, 0, e0.L, a);
        Edges l0 = e0;                                         // no landmark either
        l0.L = 0;
        const BaEdgeIndex b = l0.index(0, 0, 1);
        check("L = 0", l0, 0, 0, b);
        printf("e0_E=%d e0_pt_first_size=%zu e0_pt_first_max=%d l0_pt_first_size=%zu l0_pt_first0=%d\n", a.E, a.pt_first.size(),
               *std::max_element(a.pt_first.begin(), a.pt_first.end()), b.pt_first.size(), b.pt_first[0]);
    } else if (mode == "range") {
        long long got[2][2];
        for (int v = 0; v < 2; v++) {
            Edges bad = g;
            if (v == 0) { bad.pose[9] = bad.P; bad.pt[23] = -1; }          // a keyframe index past the end, below it a negative landmark
            else { bad.pt[9] = bad.L; bad.pose[23] = -1; }
            got[v][0] = bad.index(0, bad.L, 1).out_of_range;
            got[v][1] = bad.index(0, bad.L, 8).out_of_range;
        }
        printf("a_1thread=%lld a_8threads=%lld b_1thread=%lld b_8threads=%lld\n", got[0][0], got[0][1], got[1][0], got[1][1]);
    } else if (mode == "threads") {
        const char* what = "threads";
        const Edges s = g.shuffled(9);
        same("base, sorted", g.index(0, g.L, 1), g.index(0, g.L, 8));
        same("base, shuffled", s.index(0, s.L, 1), s.index(0, s.L, 8));
        same("base, shard", s.index(4, 9, 1), s.index(4, 9, 8));
        Edges rot = g;                                         // in order inside every one of the 8 slices, out of order where slice 3 meets slice 4
        {
            const int E = g.E(), cutpos = (int)ba_index_slice(E, 4, 8).first, k0 = E - cutpos;
            for (int k = 0; k < E; k++) { const int e = (k + k0) % E; rot.pose[k] = g.pose[e]; rot.pt[k] = g.pt[e]; }
            REQUIRE(rot.pt[cutpos] < rot.pt[cutpos - 1]);
        }
        const BaEdgeIndex r8 = rot.index(0, rot.L, 8);
        check("disorder at a slice boundary, 8 threads", rot, 0, rot.L, r8);
        REQUIRE(!r8.direct);
        same("disorder at a slice boundary", rot.index(0, rot.L, 1), r8);
        Edges five = g;                                        // fewer edges than threads: some slices are empty
        five.pose.resize(5); five.pt.resize(5); five.obs.resize(10); five.info.resize(5);
        const BaEdgeIndex f8 = five.index(0, five.L, 8);
        check("E = 5, 8 threads", five, 0, five.L, f8);
        same("E = 5", five.index(0, five.L, 1), f8);
        const Edges big = random_case(50, 3000, 20000, 5);
        const BaEdgeIndex b1 = big.index(0, big.L, 1), b8 = big.index(0, big.L, 8);
        check("random list, 8 threads", big, 0, big.L, b8);
        same("random list", b1, b8);
        Edges bs = big;                                        // the same list in order: the threaded sortedness scan and the direct path
        {
            std::vector<int> o(big.E());
            std::iota(o.begin(), o.end(), 0);
            std::stable_sort(o.begin(), o.end(), [&](int a, int b) { return big.pt[a] != big.pt[b] ? big.pt[a] < big.pt[b] : big.pose[a] < big.pose[b]; });
            for (int k = 0; k < big.E(); k++) { bs.pose[k] = big.pose[o[k]]; bs.pt[k] = big.pt[o[k]]; }
        }
        const BaEdgeIndex s8 = bs.index(0, bs.L, 8);
        check("random list in order, 8 threads", bs, 0, bs.L, s8);
        REQUIRE(s8.direct);
        same("random list in order", bs.index(0, bs.L, 1), s8);
        printf("threads_ok=1 big_edges=%d big_direct=%d\n", big.E(), (int)b8.direct);
    } else {
        fprintf(stderr, "usage: ba_index_check order | shard | all_fixed | empty | range | threads\n");
        return 2;
    }
    return 0;
}
