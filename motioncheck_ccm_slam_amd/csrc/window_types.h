// window_types.h -- the host side of the windowed matchers, shared by the host translation units that drive them: match_window_host.cpp
// (host arrays per call), frame_window_host.cpp (frame handles; mpt_track_host.cpp goes through its frame_window_dev) and
// mpt_sim3_host.cpp (keyframe handles and the map-point table).  The device structures and launchers are match_types.h.
#pragma once
#include <vector>
#include "ccm_internal.h"
#include "match_types.h"

// The queries of one call in device memory and the buffers their candidate lists go to: one frame (`grid`), or, with `grids`, a table of
// frames in device memory and each query's frame q_kf.
struct WinLists {
    WinGrid grid; const WinGrid* grids; const int* q_kf;
    int nq;
    const float* qx; const float* qy; const float* qr; const int* minl; const int* maxl; const uint8_t* qdesc;
    DevBuf* ci; DevBuf* cd; DevBuf* cn;          // [nq][cap], [nq][cap], [nq]: reserved by the launch
};
// k_window_candidates at `cap` entries a list
int window_lists_launch(ccm_ctx* c, const WinLists& L, int cap);
// The lists on the host for the host acceptance loops, `cap` grown from its first value until every list fits (rare: a denser window
// than expected).  One wait for the stream when they fit.
struct WinHostLists { int cap; std::vector<int32_t> ci, cd, cn; };
int window_lists_host(ccm_ctx* c, const WinLists& L, WinHostLists& H);

// The order-dependent acceptance on the device: the lists at cap = 64 and k_window_greedy behind them (A without cap / ci / cd / cn: one
// problem in `mode`, or A.kfs and n_problems workgroups over frames of at most max_n features).  A list longer than `cap` makes the
// kernel report the needed length, and every problem repeats at the longest one, three attempts at most.  The site's hooks:
//   reset()        before a second attempt: what the first one may have written (flags, choices) as it came in; CCM_OK or an error
//   tail()         launches queued behind the acceptance kernel
//   fetch(status)  its own download and wait; points `status` at the 3 * n_problems status words on the host; CCM_OK or an error
// On CCM_OK `*status` holds the words of the successful attempt ([3k] = matches of problem k).
template <class Reset, class Tail, class Fetch>
int window_greedy_drive(ccm_ctx* c, const WinLists& L, GreedyArgs A, int mode, int n_problems, int max_n, Reset&& reset, Tail&& tail, Fetch&& fetch,
                        const int** status)
{
    int cap = 64, rc;
    for (int attempt = 0; attempt < 3; attempt++) {
        if ((attempt && (rc = reset())) || (rc = window_lists_launch(c, L, cap))) return rc;
        A.cap = cap; A.ci = L.ci->as<int>(); A.cd = L.cd->as<int>(); A.cn = L.cn->as<int>();
        if (A.kfs ? match_launch_window_greedy_batch(c->stream, A, n_problems, max_n) : match_launch_window_greedy(c->stream, mode, A))
            return ccm_fail(c, CCM_E_DEVICE, "k_window_greedy: LDS request refused");
        tail();
        CCM_HIP(c, hipGetLastError());
        if ((rc = fetch(status))) return rc;
        cap = 0;
        for (int k = 0; k < n_problems; k++) if ((*status)[3 * k] < 0) cap = std::max(cap, (*status)[3 * k + 1]);
        if (cap == 0) return CCM_OK;
    }
    return ccm_fail(c, CCM_E_CAPACITY, "window candidate lists keep overflowing");
}

// The host acceptance loops (the round-1 path; CCM_WINDOW_HOST_ACCEPT=1 or problems above kGreedyLdsMax) on candidate lists
// [nq][cap] with counts cn.  match[] must be pre-set to -1; occupied is updated; return nmatches.
// SearchByProjection(Frame&, map points), ORBmatcher.cpp:71-148 (kp_octave: the frame's octaves)
int window_accept_projection_host(int n_mp, const uint8_t* in_view, const int32_t* ci, const int32_t* cd, const int32_t* cn, int cap,
                                  const int32_t* kp_octave, const uint8_t* mp_has_obs, uint8_t* occupied, float nnratio, int32_t* match);
// SearchByProjection(Frame&, Frame | KeyFrame), ORBmatcher.cpp:1350-1476, :1478-1605
int window_accept_frame_host(int n_last, const uint8_t* valid, const int32_t* ci, const int32_t* cd, const int32_t* cn, int cap,
                             const uint8_t* mp_has_obs, uint8_t* occupied, int orb_dist, int check_ori, const float* last_angle,
                             const float* cur_angle, int32_t* match);
// SearchByProjection(pKF, Scw, vpPoints, vpMatched, th), ORBmatcher.cpp:388-441 (TH_LOW).  matched [features] is vpMatched as flags, updated;
// best_idx[m] (pre-set to -1) gets the accepted feature; best_dist (optional) its distance, 256 where nothing is accepted; return nmatches.
int window_accept_sim3_host(int n_mp, const uint8_t* valid, const int32_t* level, const int32_t* ci, const int32_t* cd, const int32_t* cn, int cap,
                            const int32_t* kp_octave, const uint8_t* observed, uint8_t* matched, int32_t* best_idx, int32_t* best_dist = nullptr);
// Per-query search windows (radius, r < 0 skips the query; octave range) of the host-buffer and the frame-handle entry points.
struct WinQueries { std::vector<float> qr; std::vector<int32_t> minl, maxl; };
// SearchByProjection(Frame&, map points), ORBmatcher.cpp:97-107: RadiusByViewingCos (* th unless th == 1) * scale[level], levels
// level - 1 .. level; map points not in view are skipped
WinQueries window_queries_projection(int n_mp, const uint8_t* in_view, const int32_t* level, const float* view_cos, const float* scale_factors,
                                     float th);
// SearchByProjection(Frame&, Frame | KeyFrame), ORBmatcher.cpp:1401-1405: th * scale[octave], levels octave - 1 .. octave + 1
WinQueries window_queries_frame(int n_last, const uint8_t* valid, const int32_t* last_octave, const float* scale_factors, float th);
// true when CCM_WINDOW_HOST_ACCEPT=1 (test switch)
bool window_host_accept_forced();
