// ba_table.hip -- source and sink of ccm_ba_solve_table_frames (include/ccm_hot.h "local BA on the table"): the bundle adjustment's
// observations, information values and points gathered from keyframe handles and the map-point table, and its results narrowed back
// into them.  Two plain wave64 grid-stride kernels, each launched once per call; the LM loop between them is ba_host.cpp's, unchanged.
#include "ba_launch.h"
#include "pose_camera.h"
#include <algorithm>

#define BAT_TPB 256
#define BAT_MAX_BLOCKS 2048        // beyond: the grid strides

// Items [0, E): edge k in the device's (landmark, keyframe) order, obs = mvKeysUn[f].pt and info = mvInvLevelSigma2[octave[f]] of its
// keyframe's handle, widened.  The edges of one landmark are neighbours, so a wave's reads of edge_pose / edge_feat and its writes coalesce.
// Items [E, E + L): landmark l, the table's float position widened.
__global__ __launch_bounds__(BAT_TPB) void k_ba_gather_table(BaTableArgs A)
{
    const long long n = (long long)A.E + A.L, stride = (long long)gridDim.x * BAT_TPB;
    for (long long i = (long long)blockIdx.x * BAT_TPB + threadIdx.x; i < n; i += stride) {
        if (i < A.E) {
            const BaTableKf v = A.kf[A.edge_pose[i]];
            const int f = A.edge_feat[i];
            const int o = min(max(v.oct[f], 0), A.n_levels - 1);       // (the host has checked n_levels against the handle's)
            A.obs[2 * i] = (double)v.kx[f]; A.obs[2 * i + 1] = (double)v.ky[f];
            A.info[i] = (double)A.level_info[o];
        } else {
            const long long l = i - A.E;
            const float* src = A.table_pos + 3 * (long long)A.slot[l];
            double* dst = A.points + 3 * l;
            dst[0] = (double)src[0]; dst[1] = (double)src[1]; dst[2] = (double)src[2];
        }
    }
}

// Items [0, L): landmark l narrowed (the cast of Converter::toCvMat) into its table row and into pos_out.  Items [L, L + P): keyframe
// k, when published, Tcw / Ow of its optimised pose into the handle's camera.
__global__ __launch_bounds__(BAT_TPB) void k_ba_publish_table(BaTableArgs A)
{
    const long long n = (long long)A.L + A.P, stride = (long long)gridDim.x * BAT_TPB;
    for (long long i = (long long)blockIdx.x * BAT_TPB + threadIdx.x; i < n; i += stride) {
        if (i < A.L) {
            const double* src = A.points + 3 * i;
            const float x = (float)src[0], y = (float)src[1], z = (float)src[2];
            if (A.scatter) {
                float* row = A.table_pos + 3 * (long long)A.slot[i];
                row[0] = x; row[1] = y; row[2] = z;
            }
            float* out = A.pos_out + 3 * i;
            out[0] = x; out[1] = y; out[2] = z;
        } else {
            const long long k = i - A.L;
            float* cam = A.kf[k].cam;
            if (!A.scatter || !A.publish[k] || !cam) continue;
            float T[12], O[3];
            ba_pose_to_camera(A.poses + 7 * k, T, O);
            for (int q = 0; q < 12; q++) cam[q] = T[q];
            for (int q = 0; q < 3; q++) cam[12 + q] = O[q];
        }
    }
}

static inline int bat_grid(long long n) { return (int)std::min<long long>(nblk(n, BAT_TPB), BAT_MAX_BLOCKS); }

void ba_launch_gather_table(hipStream_t s, const BaTableArgs& A)
{
    const long long n = (long long)A.E + A.L;
    if (n > 0) hipLaunchKernelGGL(k_ba_gather_table, dim3(bat_grid(n)), dim3(BAT_TPB), 0, s, A);
}
void ba_launch_publish_table(hipStream_t s, const BaTableArgs& A)
{
    const long long n = (long long)A.L + A.P;
    if (n > 0) hipLaunchKernelGGL(k_ba_publish_table, dim3(bat_grid(n)), dim3(BAT_TPB), 0, s, A);
}
