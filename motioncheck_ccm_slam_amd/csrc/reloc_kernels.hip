// reloc_kernels.hip -- device side of ccm_frame_search_by_projection_keyframe (reloc_host.cpp): the relocalisation overload
// SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) of src/ORBmatcher.cpp:1478-1605 on handles and the map-point table.
//   k_reloc_mark       the found set into the table handle's stamped where[] column
//   k_reloc_project    the first half of the loop (:1494-1539), one thread per keyframe feature: the matcher's queries
//   k_reloc_clear      the matcher's result and occupancy flags from the current frame's ids, which stay as they are
//   k_reloc_camera / k_reloc_set / k_reloc_discard
//                      ccm_frame_relocalize_candidate: the view of a search from the pose in device memory, the PnP inliers as the
//                      current frame's ids, and "the outliers lose their id" behind a pose stage
// The search and the sequential acceptance behind them are k_window_candidates / k_window_greedy in mode 2 (match_window.hip).
// Every id is checked against the table's capacity before it is used as an address.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/ccm_hot.h"
#include "reloc_types.h"
#include "mpt_device.h"
#include "pose_camera.h"

// An entry of an earlier call carries an older stamp and reads as "not found"; nothing has to be cleared.  Several entries may name
// one slot: they store the same value.
__global__ void k_reloc_mark(int n, const int* ids, int capacity, unsigned long long* where, unsigned stamp)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int s = ids[j];
    if (s >= 0 && s < capacity) where[s] = (unsigned long long)stamp << 32;
}

// Keyframe feature i is a query when it holds a point (:1498) that is not bad and not in the found set (:1500), projects inside the
// bounds, both ends included (:1513-1516), and lies inside the scale pyramid (:1526, strict on both sides).  There is no depth test in
// this overload: a point behind the camera whose projection lands inside the bounds is searched.  invz = 1.0f / PcZ: the reference
// divides in double and narrows, which for one division of two floats is the same float.  Stated deviation, as in k_tmm_project: a u or
// v that is not finite (PcZ == 0) is rejected; the reference would hand it to GetFeaturesInArea.  An id outside the table or of a slot
// that is not LIVE raises head[0] (every thread that finds one stores the same 1) and is never used as an address.  The queries stay at
// their feature's index with an act byte: the acceptance is sequential in i.  A feature that is no query gets u = v = 0, level = 0.
__global__ __launch_bounds__(RLC_TPB) void k_reloc_project(RelocArgs A, MptTable T)
{
    const int i = blockIdx.x * RLC_TPB + threadIdx.x;
    if (i >= A.n_kf) return;
    const int id = A.kf_id[i];
    const float* Tcw = A.cam ? A.cam : A.Tcw;                                      // uniform per launch either way
    const float* Ow = A.cam ? A.cam + 12 : A.Ow;
    float u = 0.0f, v = 0.0f;
    int level = 0;
    bool valid = false;
    if (id >= 0) {
        const uint8_t fl = id < T.capacity ? T.flags[id] : 0;
        if (!(fl & CCM_MP_LIVE)) A.head[0] = 1;
        else if (!(fl & CCM_MP_BAD) && (unsigned)(A.where[id] >> 32) != A.stamp) {
            const float P[3] = { T.pos[3 * (size_t)id], T.pos[3 * (size_t)id + 1], T.pos[3 * (size_t)id + 2] };
            float Pc[3];
            mpt_to_camera(Tcw, P, Pc);
            const float invz = 1.0f / Pc[2];                                       // :1508
            mpt_pinhole(A.fx, A.fy, A.cx, A.cy, Pc, invz, u, v);
            valid = fabsf(u) <= 3.402823466e+38f && fabsf(v) <= 3.402823466e+38f &&      // a NaN compares false
                    !(u < A.min_x || u > A.max_x) && !(v < A.min_y || v > A.max_y);
            if (valid) {
                const float max_d = T.max_dist[id];
                const float PO[3] = { P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2] };
                const float dist = (float)sqrt((double)PO[0] * (double)PO[0] + (double)PO[1] * (double)PO[1] + (double)PO[2] * (double)PO[2]);
                valid = !(dist < 0.8f * T.min_dist[id] || dist > 1.2f * max_d);
                if (valid) level = fuse_predict_level(max_d, dist, A.log_scale, A.n_levels);       // :1529
            }
            if (!valid) { u = 0.0f; v = 0.0f; }
        }
    }
    A.qx[i] = u; A.qy[i] = v; A.level[i] = level;
    A.qr[i] = valid ? A.th * A.scale[level] : -1.0f;                               // :1532; no query: as k_frame_prep_last leaves it
    A.minl[i] = valid ? level - 1 : 0; A.maxl[i] = valid ? level + 1 : 0;          // :1534
    A.act[i] = valid ? 1 : 0; A.qflag[i] = valid ? 1 : 0;
    if (valid) {
        const uint4* a = reinterpret_cast<const uint4*>(T.desc + (size_t)id * 32);
        uint4* b = reinterpret_cast<uint4*>(A.qdesc + (size_t)i * 32);
        b[0] = a[0]; b[1] = a[1];
    }
}

// A current feature blocks a candidate when it holds any id (:1547), whatever the slot's HAS_OBS says.  The ids are not cleared.
__global__ void k_reloc_clear(int n_cur, int n_kf, const int* head, const int* mp_id, int* out, uint8_t* flag, int* ids_out, uint8_t* act)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_cur) {
        const int id = mp_id[i];
        out[i] = -1; flag[i] = id >= 0 ? 1 : 0; ids_out[i] = id;
    }
    if (head[0] != 0 && i < n_kf) act[i] = 0;
}

// ---- ccm_frame_relocalize_candidate
__global__ void k_reloc_camera(const double* pose7, float* cam)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) ba_pose_to_camera(pose7, cam, cam + 12);
}
__global__ void k_reloc_set(int n_matched, const int* feature, const int* slot, int n_cur, int* mp_id)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_matched) return;
    const int i = feature[j];
    if (i >= 0 && i < n_cur) mp_id[i] = slot[j];
}
__global__ void k_reloc_discard(int n, int* mp_id, const uint8_t* outlier, const int* ninl, int discard_from)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || ninl[1] != 0 || ninl[0] < discard_from) return;
    if (mp_id[i] >= 0 && outlier[i]) mp_id[i] = -1;
}

void reloc_launch_camera(hipStream_t s, const double* pose7, float* cam) { hipLaunchKernelGGL(k_reloc_camera, dim3(1), dim3(64), 0, s, pose7, cam); }
void reloc_launch_set(hipStream_t s, int n_matched, const int* feature, const int* slot, int n_cur, int* mp_id)
{
    if (n_matched > 0) hipLaunchKernelGGL(k_reloc_set, dim3((n_matched + 255) / 256), dim3(256), 0, s, n_matched, feature, slot, n_cur, mp_id);
}
void reloc_launch_discard(hipStream_t s, int n, int* mp_id, const uint8_t* outlier, const int* ninl, int discard_from)
{
    if (n > 0) hipLaunchKernelGGL(k_reloc_discard, dim3((n + 255) / 256), dim3(256), 0, s, n, mp_id, outlier, ninl, discard_from);
}
void reloc_launch_mark(hipStream_t s, int n, const int* ids, int capacity, unsigned long long* where, unsigned stamp)
{
    if (n > 0) hipLaunchKernelGGL(k_reloc_mark, dim3((n + 255) / 256), dim3(256), 0, s, n, ids, capacity, where, stamp);
}
void reloc_launch_project(hipStream_t s, const RelocArgs& A, const MptTable& T)
{
    if (A.n_kf > 0) hipLaunchKernelGGL(k_reloc_project, dim3((A.n_kf + RLC_TPB - 1) / RLC_TPB), dim3(RLC_TPB), 0, s, A, T);
}
void reloc_launch_clear(hipStream_t s, int n_cur, int n_kf, const int* head, const int* mp_id, int* out, uint8_t* flag, int* ids_out, uint8_t* act)
{
    const int m = n_cur > n_kf ? n_cur : n_kf;
    if (m > 0) hipLaunchKernelGGL(k_reloc_clear, dim3((m + 255) / 256), dim3(256), 0, s, n_cur, n_kf, head, mp_id, out, flag, ids_out, act);
}
