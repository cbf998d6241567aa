// map_math_check.cpp -- csrc/map_math.h on the host: what one thread of k_cnmp_triangulate computes for a matched pair, and the baseline
// rule.  Reads blocks until the end of the input, one block per (current keyframe, neighbour).
// stdin per block:  int32 n; float ratioFactor, medianDepth; MapCam cam1, cam2 (24 floats each: fx fy cx cy invfx invfy Tcw[12] Ow[3] pad[3]);
//                   MapFeat f1[n], f2[n] (x, y, sigma2, scale)
// stdout per block: int32 skipped; int32 status[n]; float X[n][3]; float cos[n]; int32 gates[n] (map_gates alone on X, where a point exists)
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../motioncheck_ccm_slam_amd/csrc/map_math.h"

template <class T> static bool rd(T* p, size_t n) { return fread(p, sizeof(T), n, stdin) == n; }
template <class T> static void wr(const T* p, size_t n) { fwrite(p, sizeof(T), n, stdout); }

int main()
{
    static_assert(sizeof(MapCam) == 96 && sizeof(MapFeat) == 16, "layout of the blocks");
    int32_t n;
    while (rd(&n, 1)) {
        float ratioFactor, medianDepth;
        MapCam c1, c2;
        if (n < 0 || !rd(&ratioFactor, 1) || !rd(&medianDepth, 1) || !rd(&c1, 1) || !rd(&c2, 1)) return 2;
        std::vector<MapFeat> f1(n), f2(n);
        if (!rd(f1.data(), f1.size()) || !rd(f2.data(), f2.size())) return 2;
        std::vector<int32_t> status(n), gates(n);
        std::vector<float> X(3 * (size_t)n), cosp(n);
        for (int i = 0; i < n; i++) {
            status[i] = map_pair(c1, c2, f1[i], f2[i], ratioFactor, &X[3 * (size_t)i], &cosp[i]);
            gates[i] = status[i] >= MAP_BEHIND_1 ? map_gates(c1, c2, f1[i], f2[i], ratioFactor, &X[3 * (size_t)i]) : status[i];
        }
        const int32_t skipped = map_baseline_too_short(c1.Ow, c2.Ow, medianDepth) ? 1 : 0;
        wr(&skipped, 1); wr(status.data(), status.size()); wr(X.data(), X.size()); wr(cosp.data(), cosp.size()); wr(gates.data(), gates.size());
    }
    return 0;
}
