// TEST SCAFFOLDING: the hat functions of the PCG's coarse space (csrc/ba_pcg.h) against the properties that k_pcg_coarse_build,
// k_ppcg_prec and ppcg_contribute rest on, for nfree = 1 .. 699 and the sizes around which the aggregate width changes.  The weights
// are multiples of 1 / (2A) with A a power of two, so every comparison is exact.  Prints one line of key=value pairs; exits 1 at
// the first mismatch.  (Beyond 16384 free keyframes the aggregate width is capped and the coarse dimension exceeds PCG_COARSE_MAX:
// not checked here either way.)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../motioncheck_ccm_slam_amd/csrc/ba_pcg.h"

#define REQUIRE(cond) do { if (!(cond)) { printf("FAILED nfree=%d f=%d I=%d: %s (line %d)\n", nfree, f, I, #cond, __LINE__); exit(1); } } while (0)

int main()
{
    std::vector<int> sizes;
    for (int n = 1; n <= 699; n++) sizes.push_back(n);
    for (int n : { 1999, 2000, 2048, 4095, 4096, 5000, 8191, 8192, 8193, 10000, 16384 }) sizes.push_back(n);
    int agg_seen[9] = { 0 };
    long long keyframes = 0, weights = 0;
    for (int nfree : sizes) {
        int f = -1, I = -1;
        const int agg = pcg_agg_clusters(nfree);
        REQUIRE(agg == 2 || agg == 4 || agg == 8);
        agg_seen[agg]++;
        const int A = PCG_CL * agg, nagg = (nfree + A - 1) / A;
        REQUIRE(PCG_CDOF * nagg <= PCG_COARSE_MAX);
        for (f = 0; f < nfree; f++) {
            const PcgHat h = pcg_hat(f, A, nagg);
            REQUIRE(h.w0 + h.w1 == 1.0);
            REQUIRE(0 <= h.i0 && h.i0 <= h.i1 && h.i1 < nagg);
            keyframes++;
        }
        for (I = 0; I < nagg; I++) {
            int first, last;
            pcg_hat_support(I, A, nfree, first, last);
            for (f = 0; f < nfree; f++) {
                const bool weighted = pcg_hat_weight(f, I, A, nagg) != 0.0;
                REQUIRE(weighted == (first <= f && f < last));
                weights += weighted;
            }
        }
    }
    printf("sizes=%d keyframes=%lld weights=%lld agg2=%d agg4=%d agg8=%d\n", (int)sizes.size(), keyframes, weights, agg_seen[2], agg_seen[4], agg_seen[8]);
    return 0;
}
