// pnp_math_check.cpp -- stand-alone check of csrc/pnp_math.h on the host (tests/test_pnp_solver_cpu.py builds it with
// -fsanitize=address,undefined and runs it as a child process).  compute_pose, CheckInliers and the sampling map on generic sets of
// 4, 5 and 40 correspondences, on a planar set and on all-equal points; every array is heap-allocated at its exact size.  Prints one
// line per case: name, finite (0 / 1), inliers; then "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>
#include "../../motioncheck_ccm_slam_amd/csrc/pnp_math.h"

struct View {
    const float* P3D; const float* P2D;
    void get(int i, double pw[3], double uv[2]) const
    {
        pw[0] = P3D[3 * i]; pw[1] = P3D[3 * i + 1]; pw[2] = P3D[3 * i + 2]; uv[0] = P2D[2 * i]; uv[1] = P2D[2 * i + 1];
    }
};

static uint64_t g_state = 88172645463325252ull;
static double uniform() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (g_state >> 11) * (1.0 / 9007199254740992.0); }

enum Kind { GENERIC, PLANAR, EQUAL };

static int run(const char* name, int n, Kind kind)
{
    const double K[4] = { 520.0, 515.0, 320.0, 240.0 };
    const double c = std::cos(0.3), s = std::sin(0.3);
    const double R[3][3] = { { c, 0, s }, { 0, 1, 0 }, { -s, 0, c } }, t[3] = { 0.2, -0.1, 0.5 };
    std::unique_ptr<float[]> P3D(new float[3 * n]), P2D(new float[2 * n]);
    for (int i = 0; i < n; i++) {
        double X[3] = { 4 * uniform() - 2, 3 * uniform() - 1.5, 4 + 4 * uniform() };
        if (kind == PLANAR) X[2] = 5.0 + 0.5 * X[0];
        if (kind == EQUAL) { X[0] = 0.5; X[1] = -0.25; X[2] = 6.0; }
        double Xc[3];
        for (int r = 0; r < 3; r++) Xc[r] = R[r][0] * X[0] + R[r][1] * X[1] + R[r][2] * X[2] + t[r];
        for (int d = 0; d < 3; d++) P3D[3 * i + d] = (float)X[d];
        P2D[2 * i] = (float)(K[2] + K[0] * Xc[0] / Xc[2] + uniform() - 0.5);
        P2D[2 * i + 1] = (float)(K[3] + K[1] * Xc[1] / Xc[2] + uniform() - 0.5);
    }
    std::unique_ptr<PnpMatHost> A(new PnpMatHost()), V(new PnpMatHost());
    std::unique_ptr<double[]> Rt(new double[12]), detail(new double[PNP_DETAIL]);
    pnp_compute_pose(View{ P3D.get(), P2D.get() }, n, K, *A, *V, Rt.get(), detail.get());
    bool finite = true;
    for (int k = 0; k < 12; k++) finite = finite && std::isfinite(Rt[k]);
    int inliers = 0;
    for (int i = 0; i < n; i++) inliers += pnp_inlier(Rt.get(), K, P3D[3 * i], P3D[3 * i + 1], P3D[3 * i + 2], P2D[2 * i], P2D[2 * i + 1], 5.991f);
    std::printf("%s %d %d\n", name, finite ? 1 : 0, inliers);
    // noise of half a pixel at most: a large generic set fits itself (a minimal set need not: EPnP's three beta approximations are
    // least-squares fits, not exact solutions)
    if (kind == GENERIC && (!finite || (n >= 40 && inliers < n - n / 10))) return 1;
    return 0;
}

int main()
{
    int bad = 0;
    bad += run("n4", 4, GENERIC); bad += run("n5", 5, GENERIC); bad += run("n40", 40, GENERIC);
    bad += run("planar", 12, PLANAR); bad += run("equal", 6, EQUAL);
    // the sampling map (:178-192) at its corners, min_set = 4 .. 8
    for (int ms = 4; ms <= 8; ms++) {
        std::vector<int> r(ms), idx(ms), avail;
        const int n = 11;
        for (int pass = 0; pass < 3; pass++) {
            for (int i = 0; i < ms; i++) r[i] = pass == 0 ? n - 1 - i : pass == 1 ? 0 : (i & 1) * (n - 1 - i);
            for (int i = 0; i < n; i++) avail.push_back(i);
            pnp_sample(n, ms, r.data(), idx.data());
            for (int i = 0; i < ms; i++) {
                if (idx[i] != avail[r[i]]) { std::printf("sample ms %d pass %d draw %d: %d != %d\n", ms, pass, i, idx[i], avail[r[i]]); bad++; }
                avail[r[i]] = avail.back(); avail.pop_back();
            }
            avail.clear();
        }
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
