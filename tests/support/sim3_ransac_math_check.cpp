// sim3_ransac_math_check.cpp -- csrc/sim3_ransac_math.h on the host: what k_sim3_ransac computes per hypothesis (s3r_sample, s3r_horn,
// then s3r_project and the two comparisons for every correspondence), in a loop.
// stdin:  int32 n, fix_scale, H; float K1[4], K2[4]; float X1[n][3], X2[n][3], max_err1[n], max_err2[n]; int32 draws[H][3]
// stdout: int32 sample[H][3]; float rts[H][13]; int32 count[H]; uint8 in[H][n]
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../motioncheck_ccm_slam_amd/csrc/sim3_ransac_math.h"

template <class T> static bool rd(T* p, size_t n) { return fread(p, sizeof(T), n, stdin) == n; }
template <class T> static void wr(const T* p, size_t n) { fwrite(p, sizeof(T), n, stdout); }

int main()
{
    int32_t n, fix, H; float K1[4], K2[4];
    if (!rd(&n, 1) || !rd(&fix, 1) || !rd(&H, 1) || !rd(K1, 4) || !rd(K2, 4) || n < 3 || H < 1) return 2;
    std::vector<float> X1(3 * (size_t)n), X2(X1.size()), m1(n), m2(n); std::vector<int32_t> draws(3 * (size_t)H);
    if (!rd(X1.data(), X1.size()) || !rd(X2.data(), X2.size()) || !rd(m1.data(), m1.size()) || !rd(m2.data(), m2.size()) || !rd(draws.data(), draws.size())) return 2;
    std::vector<int32_t> sample(3 * (size_t)H), count(H); std::vector<float> rts(13 * (size_t)H); std::vector<uint8_t> in((size_t)H * n);
    for (int h = 0; h < H; h++) {
        const int r[3] = { draws[3 * h], draws[3 * h + 1], draws[3 * h + 2] };
        for (int i = 0; i < 3; i++) if (r[i] < 0 || r[i] > n - 1 - i) return 3;
        int idx[3];
        s3r_sample(n, r, idx);
        float P1[3][3], P2[3][3];
        for (int i = 0; i < 3; i++)
            for (int d = 0; d < 3; d++) { P1[i][d] = X1[3 * idx[i] + d]; P2[i][d] = X2[3 * idx[i] + d]; }
        S3rXf xf;
        s3r_horn(P1, P2, fix != 0, rts.data() + 13 * (size_t)h, &xf);
        for (int i = 0; i < 3; i++) sample[3 * h + i] = idx[i];
        int cnt = 0;
        for (int g = 0; g < n; g++) {
            float p1u, p1v, p2u, p2v, u, v;
            s3r_project(nullptr, K1, X1[3 * g], X1[3 * g + 1], X1[3 * g + 2], &p1u, &p1v);
            s3r_project(nullptr, K2, X2[3 * g], X2[3 * g + 1], X2[3 * g + 2], &p2u, &p2v);
            s3r_project(xf.T12, K1, X2[3 * g], X2[3 * g + 1], X2[3 * g + 2], &u, &v);
            const float d1x = p1u - u, d1y = p1v - v;
            s3r_project(xf.T21, K2, X1[3 * g], X1[3 * g + 1], X1[3 * g + 2], &u, &v);
            const float d2x = u - p2u, d2y = v - p2v;
            const float e1 = d1x * d1x + d1y * d1y, e2 = d2x * d2x + d2y * d2y;
            const bool ok = e1 < m1[g] && e2 < m2[g];
            in[(size_t)h * n + g] = ok; cnt += ok;
        }
        count[h] = cnt;
    }
    wr(sample.data(), sample.size()); wr(rts.data(), rts.size()); wr(count.data(), count.size()); wr(in.data(), in.size());
    return 0;
}
