// init_types.h -- launch arguments and launchers of k_init_hypotheses and k_init_check_rt, shared by init_host.cpp and init_kernels.hip.
#pragma once
#include <cstdint>

#define INI_TPB   256     // threads per workgroup (4 waves) of k_init_hypotheses
#define INI_GROUP 16      // lanes that share one hypothesis' matrices
#define INI_SPB   8       // minimal sets per workgroup: 8 homographies (waves 0-1) and 8 fundamental matrices (waves 2-3)
#define INI_TILE  1024    // matches staged in LDS at a time (16 KB); more matches take several passes
#define INI_SWEEPS 10     // cyclic Jacobi sweeps over the 9x9 (a rotation whose off-diagonal entry is already negligible is skipped)
#define INI_RT_TPB 128    // threads per workgroup of k_init_check_rt
#define INI_MAX_CAND 8

struct IniDev {
    const float* m;               // [n][4]: u1, v1, u2, v2 of match i (mvKeys1[mvMatches12[i].first], mvKeys2[...second])
    const int32_t* sets;          // [iters][8] match indices (mvSets)
    int32_t n, iters, words;      // words = ceil(n / 64) mask words per set
    float T1[4], T2[4];           // Normalize: sX, sY, meanX, meanY of frame 1 / frame 2
    float inv_sigma2;             // invSigmaSquare
    float* H21; float* H12; float* F21;            // [iters][9]
    float* score_h; float* score_f;                // [iters]
    unsigned long long* mask_h; unsigned long long* mask_f;   // [iters][words], match i = bit i % 64 of word i / 64
};

struct IniCand { float R[9], t[3], O2[3], P2[12]; };           // one motion hypothesis: R, t, O2 = -R^T t, P2 = K [R | t]

struct IniRtDev {
    const float* m;               // [n][4]
    const unsigned long long* mask;                // [words]: vbMatchesInliers of the chosen model
    int32_t n, n_cand;
    float K[4];                   // fx, fy, cx, cy
    float th2;                    // 4 sigma^2
    uint8_t* flags;               // [n_cand][n]: bit 0 = counted in nGood (and vP3D written), bit 1 = vbGood
    float* cosp;                  // [n_cand][n]
    float* X;                     // [n_cand][n][3]
    IniCand cand[INI_MAX_CAND];
};

// The launchers (init_kernels.hip).  This header is also compiled without ROCm (tests/support/init_math_check.cpp), so it names the
// stream type as <hip/hip_runtime.h> declares it and does not include it.
typedef struct ihipStream_t* hipStream_t;
void init_hypotheses_launch(hipStream_t, const IniDev&);
void init_check_rt_launch(hipStream_t, const IniRtDev&);
