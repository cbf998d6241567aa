// ba_pcg.h -- what the preconditioner (ba_pcg_precond.hip) and the two PCG iterations (ba_pcg.hip, ba_ppcg.hip) share: the tunables of
// the cluster and coarse levels and the hat functions of the coarse space.  Compiles for the host without HIP
// (tests/support/ba_pcg_check.cpp states the properties the kernels rest on).  The tunables keep their #ifndef guards:
// tools/sweep_variants.sh rebuilds with -D (all three files with the same flags: they must agree on every value here).
#pragma once
#include <algorithm>

#if defined(__HIPCC__)
#define PCG_FN __host__ __device__ inline
#define PCG_MIN(a, b) min(a, b)
#define PCG_MAX(a, b) max(a, b)
#else
#define PCG_FN inline
#define PCG_MIN(a, b) std::min(a, b)
#define PCG_MAX(a, b) std::max(a, b)
#endif

// ---- cluster level (ba_pcg_precond.hip has the description)
#ifndef PCG_CL
#define PCG_CL 8               // keyframes per cluster (measured round 2: see DESIGN.md, preconditioner study on the GPU)
#endif
#ifndef PCG_XCDS
#define PCG_XCDS 8               // 1 = block rows in dispatch order (round-robin over the XCDs)
#endif
#define PCG_CN (6 * PCG_CL)

// ---- blocks of the kernels that make a residual (k_pcg_init, k_pcg_update, k_ppcg_init): one thread per scalar unknown
#define PCG_UPD_TPB 192       // 4 clusters of PCG_CN scalars: a cluster never straddles two blocks
#define PCG_UPD_KF (PCG_UPD_TPB / 6)

// ---- coarse level (ba_pcg_precond.hip has the description): aggregates of A = PCG_CL * pcg_agg_clusters() keyframes
#ifndef PCG_AGG
#define PCG_AGG 2                // clusters per aggregate up to PCG_COARSE_MAX coarse unknowns; doubled beyond (at most 8)
#endif
#define PCG_CDOF 7               // coarse unknowns per aggregate
#define PCG_COARSE_MAX 1792
// clusters per aggregate for a map of `nfree` free keyframes: the smallest of PCG_AGG, 2 PCG_AGG, ... (<= 8) that keeps the coarse
// system within PCG_COARSE_MAX unknowns (its inversion is cubic and has to fit inside one LM trial)
PCG_FN int pcg_agg_clusters(int nfree)
{
    int agg = PCG_AGG;
    while (2 * agg * PCG_CL <= 64 && PCG_CDOF * ((nfree + PCG_CL * agg - 1) / (PCG_CL * agg)) > PCG_COARSE_MAX) agg *= 2;
    return agg;
}
// the two aggregates keyframe f interpolates between, and its weights (w0 + w1 = 1)
struct PcgHat { int i0, i1; double w0, w1; };
PCG_FN PcgHat pcg_hat(int f, int A, int nagg)
{
    const double x = ((double)f + 0.5) * (1.0 / (double)A) - 0.5;  // A is a power of two: multiples of 1 / (2A), exact
    const int I = (int)(x + 1.0) - 1;                              // floor(x) for x >= -1
    const double al = x - (double)I;
    PcgHat h;
    h.i0 = PCG_MIN(PCG_MAX(I, 0), nagg - 1); h.i1 = PCG_MIN(I + 1, nagg - 1);
    h.w0 = 1.0 - al; h.w1 = al;
    if (h.i0 == h.i1) { h.w0 = 1.0; h.w1 = 0.0; }
    return h;
}
// weight of keyframe f in aggregate I
PCG_FN double pcg_hat_weight(int f, int I, int A, int nagg)
{
    const PcgHat h = pcg_hat(f, A, nagg);
    return (h.i0 == I ? h.w0 : 0.0) + (h.i1 == I ? h.w1 : 0.0);
}
// keyframes with a non-zero weight in aggregate I: [first, last)
PCG_FN void pcg_hat_support(int I, int A, int nfree, int& first, int& last)
{
    first = PCG_MAX(0, A * I - A / 2); last = PCG_MIN(nfree, A * I + A + A / 2);
}
