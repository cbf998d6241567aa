// frame_kernels.hip -- device side of the frame handles (frame_host.cpp, include/ccm_hot.h "frame handles"):
//   k_frame_build         gather of an extracted image's keypoints / descriptors (ccm_frame_from_extract) and the feature grid
//                         (Frame::AssignFeaturesToGrid / PosInGrid, src/Frame.cpp:103-118, 255-266), one workgroup per frame
//   k_frame_build_batch   the same for many extracted images in one launch, a workgroup per frame, with Frame::UndistortKeyPoints
//                         (src/Frame.cpp:277-307) fused into the gather (ccm_frame_from_extract_camera, ccm_frames_from_extract_camera)
//   k_frame_prep_last     query radius and level window of SearchByProjection(Current, Last) from the last frame's octaves
//   k_frame_scatter_ids   mvpMapPoints of the newly matched features
//   k_frame_pose_gather   the correspondences of PoseOptimizationClient in feature order (compaction, first[] on the device), the
//                         points from the caller's array or from a map-point table
//   k_frame_pose_scatter  mvbOutlier per feature
//   k_frame_kf_gather     the keyframe part: node-ordered copies of the descriptors and of what the pair tests read per feature
#include <hip/hip_runtime.h>
#include <cstdint>
#include "frame_types.h"

// PosInGrid (src/Frame.cpp:255-266) exactly as grid_build() in match_window_host.cpp: round() in float, half away from zero; features
// outside the grid get no cell.  A NaN coordinate gets none either (x86's conversion gives INT_MIN, the device's 0).
// G: what a build kernel knows of its frame's grid (FrameBuildArgs, FbFrame): n, cols, rows, min_x, min_y, inv_w, inv_h, kx, ky,
// cell_first, cell_items.
template <class G> __device__ inline int fb_cell(const G& A, float x, float y)
{
    const float fx = roundf((x - A.min_x) * A.inv_w), fy = roundf((y - A.min_y) * A.inv_h);
    if (fx != fx || fy != fy) return -1;
    const int px = (int)fx, py = (int)fy;
    return (px < 0 || px >= A.cols || py < 0 || py >= A.rows) ? -1 : px * A.rows + py;
}

// Frame::AssignFeaturesToGrid (src/Frame.cpp:103-118) by one workgroup, on the coordinates A.kx / A.ky the workgroup has written: the
// stages the build kernels share.  LDS: s_first[cells + 1] and s_fill[cells] counters, s_part[FB_TPB].  A build kernel clears s_fill,
// calls fb_count_scan (cell counts by LDS atomics, then their exclusive scan into s_first), publishes s_first as cell_first and as the
// fill positions, and calls fb_place_sort (atomic placement, then each cell's items sorted by feature index -- a cell holds a handful
// of features: the order the host build's index-order fill gives).
template <class G> __device__ __forceinline__ void fb_count_scan(const G& A, const int cells, const int tid, int* s_first, int* s_fill, int* s_part)
{
    for (int i = tid; i < A.n; i += FB_TPB) {
        const int c = fb_cell(A, A.kx[i], A.ky[i]);
        if (c >= 0) atomicAdd(&s_fill[c], 1);
    }
    __syncthreads();
    // exclusive scan of the counts: a contiguous slice of cells per thread, then a scan of the slice sums
    const int per = (cells + FB_TPB - 1) / FB_TPB, lo = min(tid * per, cells), hi = min(lo + per, cells);
    int sum = 0;
    for (int k = lo; k < hi; k++) sum += s_fill[k];
    s_part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < FB_TPB; off <<= 1) {
        const int v = tid >= off ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    int run = s_part[tid] - sum;
    for (int k = lo; k < hi; k++) { const int cnt = s_fill[k]; s_first[k] = run; run += cnt; }
    if (tid == FB_TPB - 1) s_first[cells] = s_part[FB_TPB - 1];
    __syncthreads();
}

template <class G> __device__ __forceinline__ void fb_place_sort(const G& A, const int cells, const int tid, int* s_first, int* s_fill)
{
    for (int i = tid; i < A.n; i += FB_TPB) {
        const int c = fb_cell(A, A.kx[i], A.ky[i]);
        if (c >= 0) A.cell_items[atomicAdd(&s_fill[c], 1)] = i;
    }
    __syncthreads();                       // the placement's global writes are visible to the workgroup
    for (int k = tid; k < cells; k += FB_TPB) {
        const int a = s_first[k], b = s_first[k + 1];
        for (int p = a + 1; p < b; p++) {  // insertion sort of one cell
            const int v = A.cell_items[p];
            int q = p - 1;
            while (q >= a && A.cell_items[q] > v) { A.cell_items[q + 1] = A.cell_items[q]; q--; }
            A.cell_items[q + 1] = v;
        }
    }
}

// One workgroup: the gather of an extracted image (or nothing: the host uploaded x .. desc), mp_id = -1, then the grid.
__global__ __launch_bounds__(FB_TPB) void k_frame_build(FrameBuildArgs A)
{
    extern __shared__ int fb_lds[];
    const int cells = A.cols * A.rows, tid = threadIdx.x;
    int* s_first = fb_lds;                 // [cells + 1]
    int* s_fill = fb_lds + cells + 1;      // [cells]
    __shared__ int s_part[FB_TPB];
    if (A.kps) {
        for (int i = tid; i < A.n; i += FB_TPB) {
            const ccm_keypoint k = A.kps[i];
            if (!A.keep_xy) { A.kx[i] = k.x; A.ky[i] = k.y; }
            A.oct[i] = k.octave; A.angle[i] = k.angle;
            const uint4* s = reinterpret_cast<const uint4*>(A.src_desc + (size_t)i * 32);
            uint4* d = reinterpret_cast<uint4*>(A.desc + (size_t)i * 32);
            d[0] = s[0]; d[1] = s[1];
        }
    }
    for (int i = tid; i < A.n; i += FB_TPB) A.mp_id[i] = -1;
    for (int k = tid; k < cells; k += FB_TPB) s_fill[k] = 0;
    __syncthreads();
    fb_count_scan(A, cells, tid, s_first, s_fill, s_part);
    for (int k = tid; k <= cells; k += FB_TPB) A.cell_first[k] = s_first[k];
    for (int k = tid; k < cells; k += FB_TPB) s_fill[k] = s_first[k];
    __syncthreads();
    fb_place_sort(A, cells, tid, s_first, s_fill);
}

// The Frame constructors of a batch of extracted images (ccm_frames_from_extract_camera; the single call is the batch of one): one
// workgroup per frame, blockIdx.x = frame, its record in device memory.  The gather undistorts each keypoint as it is read
// (Frame::UndistortKeyPoints, undistort.h): a thread first issues the loads of up to FB_GATHER keypoints, then
// runs their iterations, so that the FP64 chains (one division per iteration) start on data that arrived together.
// The record's pointers are read from memory, so the compiler cannot know that they point to global memory: they are cast to that
// address space once, which keeps the gather and the shared stages on global (not flat) loads and stores, as in k_frame_build.
#define FB_GATHER 4
#define FB_GLOBAL __attribute__((address_space(1)))
typedef unsigned fb_u32x4 __attribute__((ext_vector_type(4)));    // 16 bytes of a descriptor row
struct FbFrame {                           // the G of the shared stages for one record
    int n, cols, rows; float min_x, min_y, inv_w, inv_h;
    const FB_GLOBAL float* kx; const FB_GLOBAL float* ky; FB_GLOBAL int* cell_first; FB_GLOBAL int* cell_items;
};
__global__ __launch_bounds__(FB_TPB) void k_frame_build_batch(FrameBatchArgs A)
{
    extern __shared__ int fb_lds[];
    const int cells = A.cols * A.rows, tid = threadIdx.x;
    int* s_first = fb_lds;                 // [cells + 1]
    int* s_fill = fb_lds + cells + 1;      // [cells]
    __shared__ int s_part[FB_TPB];
    const FrameBatchRec* R = A.rec + blockIdx.x;
    const int n = R->n;
    const FB_GLOBAL ccm_keypoint* kps = (const FB_GLOBAL ccm_keypoint*)R->kps;
    const FB_GLOBAL fb_u32x4* src_desc = (const FB_GLOBAL fb_u32x4*)R->src_desc;
    FB_GLOBAL float* kx = (FB_GLOBAL float*)R->kx; FB_GLOBAL float* ky = (FB_GLOBAL float*)R->ky;
    FB_GLOBAL int* oct = (FB_GLOBAL int*)R->oct; FB_GLOBAL float* angle = (FB_GLOBAL float*)R->angle;
    FB_GLOBAL fb_u32x4* desc = (FB_GLOBAL fb_u32x4*)R->desc; FB_GLOBAL int* mp_id = (FB_GLOBAL int*)R->mp_id;
    for (int k = tid; k < 2 * n; k += FB_TPB) desc[k] = src_desc[k];      // the descriptor rows, 16 bytes per lane
    for (int base = tid; base < n; base += FB_TPB * FB_GATHER) {
        float x[FB_GATHER], y[FB_GATHER], ang[FB_GATHER]; int o[FB_GATHER];
#pragma unroll
        for (int j = 0; j < FB_GATHER; j++) {
            const int i = min(base + j * FB_TPB, n - 1);           // past the end: the last row again, not written below
            x[j] = kps[i].x; y[j] = kps[i].y; ang[j] = kps[i].angle; o[j] = kps[i].octave;
        }
#pragma unroll
        for (int j = 0; j < FB_GATHER; j++) {
            const int i = base + j * FB_TPB;
            if (i < n) {
                float ux = x[j], uy = y[j];
                if (A.undistort) undistort_point(A.cam, x[j], y[j], &ux, &uy);
                kx[i] = ux; ky[i] = uy; oct[i] = o[j]; angle[i] = ang[j];
            }
        }
    }
    for (int i = tid; i < n; i += FB_TPB) mp_id[i] = -1;
    for (int k = tid; k < cells; k += FB_TPB) s_fill[k] = 0;
    __syncthreads();                       // also: the gather's coordinates are visible to the workgroup
    const FbFrame F{ n, A.cols, A.rows, A.min_x, A.min_y, A.inv_w, A.inv_h, kx, ky, (FB_GLOBAL int*)R->cell_first, (FB_GLOBAL int*)R->cell_items };
    fb_count_scan(F, cells, tid, s_first, s_fill, s_part);
    for (int k = tid; k <= cells; k += FB_TPB) F.cell_first[k] = s_first[k];
    for (int k = tid; k < cells; k += FB_TPB) s_fill[k] = s_first[k];
    __syncthreads();
    fb_place_sort(F, cells, tid, s_first, s_fill);
}

// SearchByProjection(Current, Last) query set-up (ORBmatcher.cpp:1401-1405) from the last frame's octaves in HBM: the host
// computes the same in window_queries_frame() (th * scale_factors[octave] in float; levels octave-1 .. octave+1; skipped: r = -1).
__global__ void k_frame_prep_last(int nq, const uint8_t* valid, const int* oct, const float* scale, float th, float* qr, int* minl, int* maxl)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    if (!valid[i]) { qr[i] = -1.f; minl[i] = 0; maxl[i] = 0; return; }
    const int o = oct[i];
    qr[i] = th * scale[o];
    minl[i] = o - 1; maxl[i] = o + 1;
}

// mp_id[i] = src[match[i]] (or match[i] when src is null) for every matched feature; nothing when the acceptance kernel reported a
// list overflow (status[0] < 0: the host repeats the call)
__global__ void k_frame_scatter_ids(int n, const int* match, const int* src, const int* status, int* mp_id)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || (status && status[0] < 0)) return;
    const int q = match[i];
    if (q >= 0) mp_id[i] = src ? src[q] : q;
}

// One workgroup: the features with mp_id >= 0, in feature order (the loop of Optimizer.cpp:244-281), compacted by a ballot scan.
// kof[i] = the correspondence of feature i or -1.  A bad id or octave sets status[0] and leaves no correspondence (first[1] = 0),
// so the pose kernel behind it leaves the pose alone and the host reports CCM_E_ARG.  With a table (TABLE: A.pos, A.flags) a slot that is
// not LIVE is a bad id too; the flag of an id outside the table is read at slot 0 and not used.
template <bool TABLE>
__global__ __launch_bounds__(FB_TPB) void k_frame_pose_gather(PoseGatherArgs A)
{
    __shared__ int s_wave[FB_TPB / 64];
    __shared__ int s_base, s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) { s_base = 0; s_bad = 0; }
    __syncthreads();
    for (int base = 0; base < A.n; base += FB_TPB) {
        const int i = base + tid;
        const int id = i < A.n ? A.mp_id[i] : -1;
        const bool has = id >= 0;
        const int o = has ? A.oct[i] : 0;
        const bool bad = has && (id >= A.n_mp || (TABLE && !(A.flags[id < A.n_mp ? id : 0] & CCM_MP_LIVE)) || o < 0 || o >= A.n_levels);
        if (bad) s_bad = 1;
        const unsigned long long ball = __ballot(has);
        const int before = __popcll(ball & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wv] = __popcll(ball);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wv; w++) off += s_wave[w];
        const int k = off + before;
        if (i < A.n) A.kof[i] = has ? k : -1;
        if (has) {
            for (int d = 0; d < 3; d++) A.pts[3 * (size_t)k + d] = bad ? 0.0 : TABLE ? (double)A.pos[3 * (size_t)id + d] : A.xyz[3 * (size_t)id + d];
            A.obs[2 * (size_t)k] = (double)A.kx[i]; A.obs[2 * (size_t)k + 1] = (double)A.ky[i];
            A.info[k] = bad ? 0.0 : (double)A.inv_sigma2[o];
        }
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < FB_TPB / 64; w++) t += s_wave[w]; s_base += t; }
        __syncthreads();
    }
    if (tid == 0) { A.first[0] = 0; A.first[1] = s_bad ? 0 : s_base; A.status[0] = s_bad; }
}

__global__ void k_frame_pose_scatter(int n, const int* kof, const int* first, const uint8_t* outl, uint8_t* outlier)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = kof[i];
    outlier[i] = (k >= 0 && k < first[1]) ? outl[k] : 0;
}

// Position p of the node order (ccm_frame_set_bow) holds feature order[p]: its 32-byte descriptor and MapFeat {x, y,
// mvLevelSigma2[octave], mvScaleFactors[octave]} are copied there, so that a wave of k_cnmp_match_frames scanning a node range reads
// contiguous 16-byte words and not a gather through the index.
__global__ __launch_bounds__(256) void k_frame_kf_gather(KfGatherArgs A)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= A.m) return;
    const int i = A.order[p], o = A.oct[i];
    A.feat_o[p] = MapFeat{ A.kx[i], A.ky[i], A.sig2[o], A.sf[o] };
    const uint4* s = reinterpret_cast<const uint4*>(A.desc + (size_t)i * 32);
    uint4* d = reinterpret_cast<uint4*>(A.desc_o + (size_t)p * 32);
    d[0] = s[0]; d[1] = s[1];
}

size_t frame_build_lds(int cells) { return ((size_t)2 * cells + 1) * 4; }

int frame_launch_build(hipStream_t s, const FrameBuildArgs& A)
{
    const size_t lds = frame_build_lds(A.cols * A.rows);
    if (hipFuncSetAttribute((const void*)k_frame_build, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_frame_build, dim3(1), dim3(FB_TPB), lds, s, A);
    return 0;
}
int frame_launch_build_batch(hipStream_t s, int n_frames, const FrameBatchArgs& A)
{
    if (n_frames <= 0) return 0;
    const size_t lds = frame_build_lds(A.cols * A.rows);
    if (hipFuncSetAttribute((const void*)k_frame_build_batch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_frame_build_batch, dim3(n_frames), dim3(FB_TPB), lds, s, A);
    return 0;
}
void frame_launch_prep_last(hipStream_t s, int nq, const uint8_t* valid, const int* oct, const float* scale, float th, float* qr, int* minl, int* maxl)
{
    if (nq > 0) hipLaunchKernelGGL(k_frame_prep_last, dim3((nq + 255) / 256), dim3(256), 0, s, nq, valid, oct, scale, th, qr, minl, maxl);
}
void frame_launch_scatter_ids(hipStream_t s, int n, const int* match, const int* src, const int* status, int* mp_id)
{
    if (n > 0) hipLaunchKernelGGL(k_frame_scatter_ids, dim3((n + 255) / 256), dim3(256), 0, s, n, match, src, status, mp_id);
}
void frame_launch_pose_gather(hipStream_t s, const PoseGatherArgs& A)
{
    hipLaunchKernelGGL(A.pos ? k_frame_pose_gather<true> : k_frame_pose_gather<false>, dim3(1), dim3(FB_TPB), 0, s, A);
}
void frame_launch_pose_scatter(hipStream_t s, int n, const int* kof, const int* first, const uint8_t* outl, uint8_t* outlier)
{
    if (n > 0) hipLaunchKernelGGL(k_frame_pose_scatter, dim3((n + 255) / 256), dim3(256), 0, s, n, kof, first, outl, outlier);
}
void frame_launch_kf_gather(hipStream_t s, const KfGatherArgs& A)
{
    if (A.m > 0) hipLaunchKernelGGL(k_frame_kf_gather, dim3((A.m + 255) / 256), dim3(256), 0, s, A);
}
