// map_geometry_check.cpp -- csrc/map_math.h on the host: the definitions behind ccm_map_pair_geometry and ccm_scene_median_depth, and
// a rank selection that needs neither a sort nor a compaction (bit by bit over the order-preserving keys, what a workgroup can do
// with counting passes), held to the same answer.  Reads records until the end of the input.
// stdin per record:  int32 kind;
//   kind 0 (pair):   float K1[4], Tcw1[12], Ow1[3], K2[4], Tcw2[12]
//   kind 1 (median): int32 n, capacity; int32 mp_id[n]; float pos[capacity][3]; uint8 flags[capacity]; float Tcw[12]
// stdout per record: kind 0: float F12[9], epipole[2];  kind 1: float median; int32 n_depths; float median_by_bits; int32 n_depths_by_bits
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../motioncheck_ccm_slam_amd/csrc/map_math.h"

template <class T> static bool rd(T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, stdin) == n; }
template <class T> static void wr(const T* p, size_t n) { fwrite(p, sizeof(T), n, stdout); }

// The key of rank r is the largest v with #(key < v) <= r, built from the top bit down
static int median_by_bits(int n, const int32_t* mp_id, int capacity, const float* pos, const uint8_t* flags, const float* Tcw, float* median)
{
    std::vector<uint32_t> key((size_t)n);
    int m = 0;
    for (int i = 0; i < n; i++) { key[i] = map_feature_depth_key(mp_id[i], capacity, pos, flags, Tcw); m += key[i] != MAP_KEY_NONE; }
    *median = 0.0f;
    if (m == 0) return 0;
    const int r = (m - 1) / 2;
    uint32_t v = 0;
    for (int bit = 31; bit >= 0; bit--) {
        const uint32_t t = v | (1u << bit);
        int below = 0;
        for (int i = 0; i < n; i++) below += key[i] < t;
        if (below <= r) v = t;
    }
    *median = map_key_depth(v);
    return m;
}

int main()
{
    int32_t kind;
    while (fread(&kind, 4, 1, stdin) == 1) {
        if (kind == 0) {
            float K1[4], T1[12], O1[3], K2[4], T2[12], F[9], e[2];
            if (!rd(K1, 4) || !rd(T1, 12) || !rd(O1, 3) || !rd(K2, 4) || !rd(T2, 12)) return 2;
            map_pair_geometry(K1, T1, O1, K2, T2, F, e);
            wr(F, 9); wr(e, 2);
        } else if (kind == 1) {
            int32_t n, capacity;
            if (!rd(&n, 1) || !rd(&capacity, 1) || n < 0 || capacity < 0) return 2;
            std::vector<int32_t> ids((size_t)n);
            std::vector<float> pos(3 * (size_t)capacity);
            std::vector<uint8_t> flags((size_t)capacity);
            float T[12];
            if (!rd(ids.data(), ids.size()) || !rd(pos.data(), pos.size()) || !rd(flags.data(), flags.size()) || !rd(T, 12)) return 2;
            float med, med2;
            const int32_t m = map_scene_median_depth(n, ids.data(), capacity, pos.data(), flags.data(), T, &med);
            const int32_t m2 = median_by_bits(n, ids.data(), capacity, pos.data(), flags.data(), T, &med2);
            wr(&med, 1); wr(&m, 1); wr(&med2, 1); wr(&m2, 1);
        } else return 2;
    }
    return 0;
}
