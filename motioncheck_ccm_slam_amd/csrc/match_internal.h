// match_internal.h -- what the matcher's host translation units share (match_bf_host.cpp, match_bow_host.cpp, match_window_host.cpp):
// the context's device buffers and the rotation consistency check.
#pragma once
#include "frame_internal.h"
#include "match_device.h"
#include <vector>

struct WindowBufs { DevBuf kx, ky, oct, desc, cfirst, citems, qx, qy, qr, minl, maxl, qdesc, ci, cd, cn, sel_i, sel_d, is2, act, qlvl, qflag, flag, out, status, qang, fang, ev,
                           grids, qkf, gkf; };
struct MatchState {
    WindowBufs win;                             // windowed matchers
    DevBuf q, t, nqn, ntn, bi, bd, sd;          // brute force staging
    DevBuf part_best, part_second;              // per-split partial results
    DevBuf d1, d2, order2, start, len, off, dist; // BoW staging
    DevBuf order1, grp[4], bv1, bv2, ba1, ba2, taken, m12, binof, hist;   // device-side SearchByBoW
    DevBuf bowf;                                // SearchByBoW on frame handles: group ranges, taken, bin_of and derived masks per pair
};
inline MatchState* match_state(ccm_ctx* c)
{
    if (!c->match) c->match = new MatchState();
    return c->match;
}
inline WindowBufs& window_bufs(ccm_ctx* c) { return match_state(c)->win; }

// ORBmatcher::ComputeThreeMaxima, ORBmatcher.cpp:1607-1648
inline void three_maxima(const std::vector<int>* histo, int L, int& ind1, int& ind2, int& ind3)
{
    int max1 = 0, max2 = 0, max3 = 0;
    ind1 = ind2 = ind3 = -1;
    for (int i = 0; i < L; i++) {
        const int s = (int)histo[i].size();
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

// The matchers' rotation consistency check (HISTO_LENGTH 30): add() files a match under its angle difference, outliers() are the
// matches outside the three fullest bins (ComputeThreeMaxima), which the caller undoes.
struct RotHisto {
    static const int HISTO = 30;
    std::vector<int> rot[HISTO];
    void add(float r, int idx) { rot[rot_bin(r)].push_back(idx); }
    std::vector<int> outliers() const
    {
        int i1, i2, i3;
        three_maxima(rot, HISTO, i1, i2, i3);
        std::vector<int> out;
        for (int b = 0; b < HISTO; b++)
            if (b != i1 && b != i2 && b != i3) out.insert(out.end(), rot[b].begin(), rot[b].end());
        return out;
    }
};
