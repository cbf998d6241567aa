// bow_directory.h -- the node directory of a keyframe handle (ccm_frame_set_bow): the features that have a FeatureVector node, ordered
// by (node, feature index) -- the order DBoW2 fills a FeatureVector in and ORBmatcher::SearchForTriangulation (ORBmatcher.cpp:739-805)
// walks it -- with the distinct nodes and the first position of each.  Plain C++ with no HIP include: frame_host.cpp uses it and
// tests/support/bow_directory_check.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

struct BowDirectory {
    std::vector<int32_t> order;   // [n_with_node] feature indices by (node, index)
    std::vector<int32_t> nodes;   // [n_nodes] distinct nodes, ascending
    std::vector<int32_t> first;   // [n_nodes + 1] the features of nodes[j] are order[first[j] .. first[j + 1])
};

// node[i] = FeatureVector node of feature i, negative = none.  Runs at keyframe rate over n ~ 2000 integers.
inline void bow_directory_build(const int32_t* node, int n, BowDirectory& D)
{
    D.order.clear(); D.nodes.clear(); D.first.clear();
    for (int i = 0; i < n; i++) if (node[i] >= 0) D.order.push_back(i);
    std::stable_sort(D.order.begin(), D.order.end(), [node](int32_t a, int32_t b) { return node[a] < node[b]; });
    for (size_t p = 0; p < D.order.size(); p++)
        if (p == 0 || node[D.order[p]] != node[D.order[p - 1]]) { D.nodes.push_back(node[D.order[p]]); D.first.push_back((int32_t)p); }
    D.first.push_back((int32_t)D.order.size());
}
