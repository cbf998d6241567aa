// bow_directory_dev.h -- arguments of k_bow_directory and the launchers of bow_kernels.hip, shared with their callers (bow_host.cpp,
// frame_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// Largest frame whose node directory the single-workgroup kernel builds (its nodes and their sorted copy live in LDS, 32 KiB in
// all); a frame above it gets the host build of bow_directory.h.
constexpr int kBowDirMax = 4096;

struct BowDirArgs {
    int n;
    const int* leaf; const int* nid;            // k_voc_transform's leaf_node and node_id; leaf == nullptr: no feature has a node
    const uint8_t* pos;                         // per vocabulary node: weight > 0
    int* node;                                  // [n] out: FeatureVector node per feature, -1 = none
    int* node_copy;                             // optional second copy of node (may alias nid), or nullptr
    int* order; int* nodes; int* first;         // out: the directory, room for n, n and n + 1 entries
    int* counts;                                // out: { features with a node, distinct nodes }
};
int bow_launch_directory(hipStream_t, const BowDirArgs&);   // nonzero: n outside [0, kBowDirMax], nothing launched
void bow_launch_transform(hipStream_t, const uint8_t* feat, int n, const int* node_first, const int* node_count, const uint8_t* slot_desc,
                          const int* slot_node, const int* node_word, int nid_level, int max_depth, int* word_id, int* leaf_node, int* node_id);
void bow_launch_distinctive(hipStream_t, const uint8_t* desc, const long long* first, const int* count, int n_points, int* best);
