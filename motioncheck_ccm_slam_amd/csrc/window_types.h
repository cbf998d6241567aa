// window_types.h -- the host side of the windowed matchers, shared by the host translation units that drive them: match_window_host.cpp
// (host arrays per call) and frame_host.cpp / mpt_host.cpp (frame handles).  The device structures and launchers are match_types.h.
#pragma once
#include <vector>
#include "match_types.h"

// The host acceptance loops (the round-1 path; CCM_WINDOW_HOST_ACCEPT=1 or problems above kGreedyLdsMax) on candidate lists
// [nq][cap] with counts cn.  match[] must be pre-set to -1; occupied is updated; return nmatches.
// SearchByProjection(Frame&, map points), ORBmatcher.cpp:71-148 (kp_octave: the frame's octaves)
int window_accept_projection_host(int n_mp, const uint8_t* in_view, const int32_t* ci, const int32_t* cd, const int32_t* cn, int cap,
                                  const int32_t* kp_octave, const uint8_t* mp_has_obs, uint8_t* occupied, float nnratio, int32_t* match);
// SearchByProjection(Frame&, Frame | KeyFrame), ORBmatcher.cpp:1350-1476, :1478-1605
int window_accept_frame_host(int n_last, const uint8_t* valid, const int32_t* ci, const int32_t* cd, const int32_t* cn, int cap,
                             const uint8_t* mp_has_obs, uint8_t* occupied, int orb_dist, int check_ori, const float* last_angle,
                             const float* cur_angle, int32_t* match);
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
