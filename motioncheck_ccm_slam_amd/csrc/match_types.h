// match_types.h -- kernel argument structures, launch constants and launchers of the matcher's CDNA4 (gfx950) kernels, shared with the
// host translation units that launch into them (match_*_host.cpp; frame_window_host.cpp, mpt_fuse_host.cpp and mpt_sim3_host.cpp through
// window_types.h).
//
// 256-bit Hamming matching, one file per kernel family:
//   match_bf.hip      k_hamming_mfma    brute-force best / second-best per query on the matrix cores (<= 2048 train rows per pair):
//                                       bits as FP4 operands of the block-scaled matrix instruction
//                     k_hamming_bf      the same on the vector ALU (any size): inner loop of ORBmatcher::SearchByBoW,
//                     + k_hamming_merge cslam/src/ORBmatcher.cpp:224-245, with every feature in one vocabulary node
//                     k_hamming_ranges  distances of each side-1 feature to its vocabulary node's side-2 features (the
//                                       DescriptorDistance calls of SearchByBoW / SearchForTriangulation; acceptance on the host)
//   match_bow.hip     k_bow_greedy, k_bow_filter (+ _batch, k_bow_groups, k_bow_invert on frame handles)   SearchByBoW, :178-306, :565-698
//   match_window.hip  k_window_candidates, k_window_select, k_window_greedy   Frame::GetFeaturesInArea and the acceptance of
//                                       SearchByProjection / Fuse / SearchBySim3, :71-148 and following
// match_device.h holds the device helpers that more than one of them uses.  The host side is split the same way (match_bf_host.cpp,
// match_bow_host.cpp, match_window_host.cpp; shared state in match_internal.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

void match_launch_bf(hipStream_t, const uint8_t* q, long long q_pair_bytes, const uint8_t* t, long long t_pair_bytes,
                     int nq, int nt, int n_pairs, const int* nq_n, const int* nt_n, int n_split,
                     unsigned* part_best, int* part_second, int* bi, int* bd, int* sd);
void match_launch_ranges(hipStream_t, const uint8_t* d1, const uint8_t* d2, const int* order2, const int* start,
                         const int* len, const long long* off, int n1, unsigned short* dist);
void match_launch_fp4_tile(hipStream_t, const unsigned* a, const unsigned* b, const float* c, float* out);

// SearchByBoW on the device: k_bow_greedy and k_bow_filter
struct BowDev {
    int n_groups, n1;
    const int* ga; const int* gae; const int* gb; const int* gbe;     // per group: ranges in ord1 / ord2
    const int* ord1; const int* ord2;
    const uint8_t* d1; const uint8_t* d2;                             // descriptors, 16-byte aligned
    const uint8_t* valid1; const uint8_t* valid2;                     // valid2 may be null
    const float* angle1; const float* angle2;
    uint8_t* taken; int* match12; int* bin_of; int* hist;             // hist[30] + [30] = kept count
    float nnratio; int th, strict_th, check_ori;
};
void match_launch_bow(hipStream_t, const BowDev&);

// SearchByBoW on frame handles: one record per pair; the batched forms take the pair from blockIdx.y
struct BowFrameRec {
    BowDev B;                                        // n_groups = side 1's distinct nodes; ga .. gbe, taken, match12, hist are filled by k_bow_groups
    const int* nodes1; const int* first1;            // side 1's directory
    const int* nodes2; const int* first2;            // side 2's
    int n_nodes2, n2;
    const int* mp1; const int* mp2;                  // the handles' mp_id
    uint8_t* v1; uint8_t* v2;                        // non-null: B.valid1 / B.valid2 are these, derived here as mp_id >= 0
    int* match21;                                    // Frame overload: [n2], cleared here and filled by k_bow_invert; else null
};
void match_launch_bow_groups(hipStream_t, const BowFrameRec& one, const BowFrameRec* recs, int n_recs, int max_threads);
void match_launch_bow_batch(hipStream_t, const BowFrameRec* recs, int n_recs, int n_groups);
void match_launch_bow_invert(hipStream_t, const BowFrameRec&, int min_matches, int* mp_id2);

// The windowed matchers: a frame's features and its grid (Frame::GetFeaturesInArea)
struct WinGrid {
    int n, cols, rows;
    float min_x, min_y, inv_w, inv_h;
    const float* kx; const float* ky; const int* oct; const uint8_t* desc;
    const int* cell_first; const int* cell_items;
};
void match_launch_window(hipStream_t, const WinGrid&, int nq, const float* qx, const float* qy, const float* qr, const int* minl,
                         const int* maxl, const uint8_t* qdesc, int cap, int* ci, int* cd, int* cn);
void match_launch_window_batch(hipStream_t, const WinGrid* grids, const int* q_kf, int nq, const float* qx, const float* qy, const float* qr, const int* minl,
                               const int* maxl, const uint8_t* qdesc, int cap, int* ci, int* cd, int* cn);
void match_launch_window_select(hipStream_t, const WinGrid&, int nq, const float* qx, const float* qy, const float* qr, const int* minl,
                                const int* maxl, const uint8_t* qdesc, const float* inv_sigma2, int accept_th, int* best_idx, int* best_dist);
void match_launch_window_select_batch(hipStream_t, const WinGrid* grids, const int* q_kf, int nq, const float* qx, const float* qy, const float* qr,
                                      const int* minl, const int* maxl, const uint8_t* qdesc, const float* inv_sigma2, int accept_th, int* best_idx, int* best_dist);

// k_window_greedy: the acceptance loops of the windowed matchers in one workgroup
struct GreedyKf { int q0, nq, f0, n; };
struct GreedyArgs {
    int nq, n, cap;
    const int* ci; const int* cd; const int* cn;      // candidate lists [nq][cap], counts
    const uint8_t* active;                            // mbTrackInView && !isBad  /  passed the projection tests
    const int* qlevel; const int* oct;                // predicted level per point, octave per feature
    const uint8_t* qflag;                             // Observations() > 0  /  already observed in the keyframe
    uint8_t* flag;                                    // in/out per feature: occupied / matched
    float nnratio;
    int* out;                                         // MODE 0 / 2: match[feature] = point; MODE 1: best_idx[point] = feature
    int* status;                                      // [0] matches (or -1: a list overflowed), [1] longest list, [2] most rounds a wave needed
    // MODE 2: acceptance threshold, rotation check and its inputs; ev[point] = accepted feature << 8 | rotation bin (or -1)
    int orb_dist, check_ori; const float* q_angle; const float* f_angle; int* ev;
    // batch (MODE 1, ccm_search_by_projection_sim3_batch): workgroup k works on keyframe k -- queries kfs[k].q0 .. +nq of the per-query
    // arrays, features kfs[k].f0 .. +n of the per-feature arrays, status words 3k .. 3k+2; nullptr = one problem, as described above
    const GreedyKf* kfs;
};
// LDS the single-workgroup acceptance kernel may ask for (claim + flag per feature, one byte per query); larger problems take the
// host acceptance loops (window_types.h)
static const size_t kGreedyLdsMax = 150 * 1024;
size_t match_window_greedy_lds(int n, int nq);
int match_launch_window_greedy(hipStream_t, int mode, const GreedyArgs&);
int match_launch_window_greedy_batch(hipStream_t, const GreedyArgs&, int n_kf, int max_n);
