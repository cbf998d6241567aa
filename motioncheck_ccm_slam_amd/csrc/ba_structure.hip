// ba_structure.hip -- block structure of the reduced camera system, made once per problem: the (landmark, pose-pair) contributions
// are enumerated, sorted by their target 6x6 block (rocPRIM radix sort, stable) and cut into one segment per block; the blocks get
// their coordinates and symmetric row lists.  ba_schur.hip sums the segments in every LM trial and says why it is a gather.
// The only file that includes rocPRIM (its scan and sort instantiations are most of the library's compile time).
#include <hip/hip_runtime.h>
#include <cstring>                     // rocPRIM uses memset without including it
#include <rocprim/rocprim.hpp>
#include <cstdint>
#include "ba_types.h"
#include "ba_launch.h"

// number of (a <= b) pairs among a landmark's edges whose pose is free
__global__ __launch_bounds__(256) void k_sp_pair_count(BaDev D, int* __restrict__ cnt)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= D.L) return;
    int kf = 0;
    for (int e = D.pt_first[l]; e < D.pt_first[l + 1]; e++) kf += D.free_of[D.edge_pose[e]] >= 0;
    cnt[l] = kf * (kf + 1) / 2;
}
void sp_launch_pair_count(hipStream_t s, const BaDev& D, int* cnt) { hipLaunchKernelGGL(k_sp_pair_count, dim3(nblk(D.L, 256)), dim3(256), 0, s, D, cnt); }

// enumerate the pairs: key = f_a * nfree + f_b (f_a <= f_b because edges are sorted by pose), value = (ea, eb), in the order of a walk
// through the landmark's triangle row by row.  SP_PF_LANES lanes per landmark: they collect the landmark's free edges in LDS (in edge
// order, by ballot) and write the triangle's entries i = g, g + SP_PF_LANES, ... -- neighbouring lanes, neighbouring entries.  (One
// thread per landmark left every lane of a wave storing into a region of its own, 46 entries apart at config 5: 260 us for 110 MB;
// a lane per ROW of the triangle, re-reading the edges from global memory: 153 us.)  A landmark with more than SP_PF_CAP free edges
// takes the row form.
#define SP_PF_LANES 8
#define SP_PF_CAP 48
__global__ __launch_bounds__(256) void k_sp_pair_fill(BaDev D, const int* __restrict__ off, unsigned* __restrict__ key,
                                                      unsigned long long* __restrict__ val)
{
    __shared__ int2 fl[256 / SP_PF_LANES][SP_PF_CAP];
    const int gt = blockIdx.x * 256 + threadIdx.x;
    const int l = gt / SP_PF_LANES, g = gt - l * SP_PF_LANES;
    if (l >= D.L) return;
    int2* mine = fl[threadIdx.x / SP_PF_LANES];
    const int e0 = D.pt_first[l], e1 = D.pt_first[l + 1];
    const int shift = (threadIdx.x & 63) - g;                        // first lane of the group inside its wave
    int kf = 0;
    for (int eb = e0; eb < e1; eb += SP_PF_LANES) {                  // (the same trip count for the lanes of a group)
        const int e = eb + g;
        const int fr = e < e1 ? D.free_of[D.edge_pose[e]] : -1;
        const unsigned gm = (unsigned)(__ballot(fr >= 0) >> shift) & ((1u << SP_PF_LANES) - 1u);
        if (fr >= 0) {
            const int pos = kf + __popc(gm & ((1u << g) - 1u));
            if (pos < SP_PF_CAP) mine[pos] = make_int2(e, fr);
        }
        kf += __popc(gm);
    }
    const int base = off[l];
    if (kf <= SP_PF_CAP) {
        const int T = kf * (kf + 1) / 2;
        int r = 0, row_start = 0, row_len = kf;
        for (int i = g; i < T; i += SP_PF_LANES) {
            while (i >= row_start + row_len) { row_start += row_len; row_len--; r++; }
            const int2 ea = mine[r], eb2 = mine[r + (i - row_start)];
            key[base + i] = (unsigned)ea.y * (unsigned)D.nfree + (unsigned)eb2.y;
            val[base + i] = ((unsigned long long)(unsigned)ea.x << 32) | (unsigned)eb2.x;
        }
        return;
    }
    int r = 0;
    for (int a = e0; a < e1; a++) {
        const int fa = D.free_of[D.edge_pose[a]];
        if (fa < 0) continue;
        if (r % SP_PF_LANES == g) {
            int p = base + r * kf - r * (r - 1) / 2;
            for (int b = a; b < e1; b++) {
                const int fb = D.free_of[D.edge_pose[b]];
                if (fb < 0) continue;
                key[p] = (unsigned)fa * (unsigned)D.nfree + (unsigned)fb;
                val[p] = ((unsigned long long)(unsigned)a << 32) | (unsigned)b;
                p++;
            }
        }
        r++;
    }
}
void sp_launch_pair_fill(hipStream_t s, const BaDev& D, const int* off, unsigned* key, unsigned long long* val)
{ hipLaunchKernelGGL(k_sp_pair_fill, dim3(nblk((long long)SP_PF_LANES * D.L, 256)), dim3(256), 0, s, D, off, key, val); }

__global__ __launch_bounds__(256) void k_sp_mark(const unsigned* __restrict__ key, long long np, int nfree, uint8_t* __restrict__ map)
{
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i < np) map[key[i]] = 1;
    if (i < nfree) map[(unsigned)i * (unsigned)nfree + (unsigned)i] = 1;      // every free pose owns its diagonal block
}
void sp_launch_mark(hipStream_t s, const unsigned* key, long long np, int nfree, uint8_t* map)
{ const long long m = np > nfree ? np : nfree; hipLaunchKernelGGL(k_sp_mark, dim3(nblk(m, 256)), dim3(256), 0, s, key, np, nfree, map); }

__global__ __launch_bounds__(256) void k_sp_block_coords(const uint8_t* __restrict__ map, const int* __restrict__ id, long long n2, int nfree,
                                                         int* __restrict__ blk_row, int* __restrict__ blk_col, int* __restrict__ diag_id)
{
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n2 || !map[i]) return;
    const int r = (int)(i / nfree), c = (int)(i - (long long)r * nfree);
    blk_row[id[i]] = r; blk_col[id[i]] = c;
    if (r == c) diag_id[r] = id[i];
}
void sp_launch_block_coords(hipStream_t s, const uint8_t* map, const int* id, long long n2, int nfree, int* br, int* bc, int* diag)
{ hipLaunchKernelGGL(k_sp_block_coords, dim3(nblk(n2, 256)), dim3(256), 0, s, map, id, n2, nfree, br, bc, diag); }

__global__ __launch_bounds__(256) void k_sp_pair_block(const unsigned* __restrict__ key, const int* __restrict__ id, long long np, unsigned* __restrict__ out)
{
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i < np) out[i] = (unsigned)id[key[i]];
}
void sp_launch_pair_block(hipStream_t s, const unsigned* key, const int* id, long long np, unsigned* out)
{ if (np > 0) hipLaunchKernelGGL(k_sp_pair_block, dim3(nblk(np, 256)), dim3(256), 0, s, key, id, np, out); }

__global__ __launch_bounds__(256) void k_sp_seg_bounds(const unsigned* __restrict__ sk, long long np, int* __restrict__ start, int* __restrict__ end)
{
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= np) return;
    if (i == 0 || sk[i] != sk[i - 1]) start[sk[i]] = (int)i;
    if (i == np - 1 || sk[i] != sk[i + 1]) end[sk[i]] = (int)i + 1;
}
void sp_launch_seg_bounds(hipStream_t s, const unsigned* sk, long long np, int* st, int* en)
{ if (np > 0) hipLaunchKernelGGL(k_sp_seg_bounds, dim3(nblk(np, 256)), dim3(256), 0, s, sk, np, st, en); }

// symmetric row lists for the mat-vec: entry key = row * nfree + col, value = block id | transposed << 31
__global__ __launch_bounds__(256) void k_sp_row_entries(const int* __restrict__ blk_row, const int* __restrict__ blk_col, int nb, int nfree,
                                                        unsigned* __restrict__ key, unsigned* __restrict__ val)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    const unsigned r = blk_row[i], c = blk_col[i];
    key[2 * i] = r * (unsigned)nfree + c; val[2 * i] = (unsigned)i;
    key[2 * i + 1] = r == c ? 0xFFFFFFFFu : c * (unsigned)nfree + r;          // diagonal blocks appear once
    val[2 * i + 1] = (unsigned)i | 0x80000000u;
}
void sp_launch_row_entries(hipStream_t s, const int* br, const int* bc, int nb, int nfree, unsigned* key, unsigned* val)
{ hipLaunchKernelGGL(k_sp_row_entries, dim3(nblk(nb, 256)), dim3(256), 0, s, br, bc, nb, nfree, key, val); }
__global__ __launch_bounds__(256) void k_sp_row_ptr(const unsigned* __restrict__ skey, int n_ent, int nfree, int* __restrict__ row_ptr)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ent) return;
    const unsigned k = skey[i];
    if (k == 0xFFFFFFFFu) return;
    const int r = (int)(k / (unsigned)nfree);
    const bool first = i == 0 || (int)(skey[i - 1] / (unsigned)nfree) != r;
    const bool last = i == n_ent - 1 || skey[i + 1] == 0xFFFFFFFFu || (int)(skey[i + 1] / (unsigned)nfree) != r;
    if (first) row_ptr[2 * r] = i;
    if (last) row_ptr[2 * r + 1] = i + 1;
}
void sp_launch_row_ptr(hipStream_t s, const unsigned* skey, int n_ent, int nfree, int* row_ptr)
{ hipLaunchKernelGGL(k_sp_row_ptr, dim3(nblk(n_ent, 256)), dim3(256), 0, s, skey, n_ent, nfree, row_ptr); }

// ---- scans and sorts (rocPRIM)
struct U8ToInt { __host__ __device__ int operator()(uint8_t v) const { return v ? 1 : 0; } };
size_t sp_scan_temp_bytes(size_t n)
{
    size_t a = 0, b = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (const int*)nullptr, (int*)nullptr, 0, n, rocprim::plus<int>());
    auto it = rocprim::make_transform_iterator((const uint8_t*)nullptr, U8ToInt());
    (void)rocprim::exclusive_scan(nullptr, b, it, (int*)nullptr, 0, n, rocprim::plus<int>());
    return a > b ? a : b;
}
hipError_t sp_scan_int(hipStream_t s, void* tmp, size_t tmp_bytes, const int* in, int* out, size_t n)
{
    return rocprim::exclusive_scan(tmp, tmp_bytes, in, out, 0, n, rocprim::plus<int>(), s);
}
hipError_t sp_scan_flags(hipStream_t s, void* tmp, size_t tmp_bytes, const uint8_t* in, int* out, size_t n)
{
    auto it = rocprim::make_transform_iterator(in, U8ToInt());
    return rocprim::exclusive_scan(tmp, tmp_bytes, it, out, 0, n, rocprim::plus<int>(), s);
}
size_t sp_sort_temp_bytes(size_t n)
{
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned long long*)nullptr,
                                    (unsigned long long*)nullptr, n, 0, 32);
    (void)rocprim::radix_sort_pairs(nullptr, b, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr, n, 0, 32);
    return a > b ? a : b;
}
hipError_t sp_sort_u64(hipStream_t s, void* tmp, size_t tmp_bytes, const unsigned* kin, unsigned* kout, const unsigned long long* vin,
                       unsigned long long* vout, size_t n, int bits)
{
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, kin, kout, vin, vout, n, 0, bits, s);
}
hipError_t sp_sort_u32(hipStream_t s, void* tmp, size_t tmp_bytes, const unsigned* kin, unsigned* kout, const unsigned* vin, unsigned* vout, size_t n)
{
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, kin, kout, vin, vout, n, 0, 32, s);
}
