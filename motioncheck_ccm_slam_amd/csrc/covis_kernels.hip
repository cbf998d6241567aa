// covis_kernels.hip -- the device side of the covisibility index (covis_host.cpp): for a batch of stored keyframes, the counter of
// KeyFrame::UpdateConnections (src/KeyFrame.cpp:644-662) against every stored keyframe and the per-point observer count of
// LocalMapping::KeyFrameCullingV3 (src/Mapping.cpp:818-855), both from "which keyframe holds which table slot".
//
// A query's COUNTING entries (it holds a point, and the table says that point is alive) go into an open-addressing hash: linear
// probing, at most half full, the key is the table slot.  A slot the query holds twice is inserted twice, so a probe walks to the
// first empty cell and meets every match: the pair count of the header.  The hash lies in LDS up to COVIS_LDS_FEATURES features
// (every workgroup builds its own copy: 2048 inserts against the 32000 probes of its chunk); a longer query is hashed once in
// global scratch by k_covis_build and the same code probes it there.
//
//   k_covis_weights     one workgroup per (chunk of COVIS_CHUNK stored slots, query); a wave takes one stored record at a time, its
//                       lanes stride over the record's slots (coalesced 4-byte loads, COVIS_UNROLL chunks of 64 in flight) and probe
//                       the hash; the lanes' pair counts are summed over the wave and lane 0 stores weights[q][s].  Every cell of
//                       weights has exactly one owner, so nothing clears the array and there are no atomics on it.
//   k_covis_redundancy  one workgroup of 16 waves per query, over the records whose weight is > 0 only, dealt to the waves in turn
//                       (one wave per range of slots measured 0.79 ms for one query of the 2000-keyframe map: a keyframe's forty
//                       neighbours have neighbouring slots and fell to one wave).  A match whose octave passes adds 1 to the matched
//                       entry's counter, which shares a word with the entry's octave (octave << 24 | count) and stops at th_obs, as
//                       the reference's loop breaks there (:844).  The sums are integers: the order does not matter.
#include "covis_types.h"

#define COVIS_TPB (64 * COVIS_WAVES)
#define COVIS_RED_TPB 1024                 // k_covis_redundancy: one workgroup per query, so it is a large one (16 waves share the records)
#define COVIS_UNROLL 4                     // chunks of 64 record features a wave probes side by side in one trip

extern __shared__ __attribute__((aligned(16))) int32_t covis_lds[];

// lowbias32: every input bit reaches every output bit, so slots in strides of 2^k spread as well as random ones do
__device__ __forceinline__ uint32_t covis_hash(int32_t slot)
{
    uint32_t x = (uint32_t)slot;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ bool covis_counts(const CovisQuery& a, int32_t v)
{
    if ((uint32_t)v >= 0x7fffffffu) return false;                             // negative: no point; INT32_MAX: no table slot yet
    if (!a.flags) return true;
    return v < a.flags_capacity && (a.flags[v] & (COVIS_MP_LIVE | COVIS_MP_BAD)) == COVIS_MP_LIVE;
}

// The whole workgroup: clears `cells` cells, inserts the counting entries of record r and returns (to every thread) their number
// in cnt[0] and the number of entries that hold a point but do not count in cnt[1].  cnt: two LDS words, or nullptr when nobody
// asks.  val may be nullptr.
__device__ __forceinline__ void covis_build(const CovisQuery& a, const RecordSlot r, int cells, int32_t* key, int32_t* val, int32_t* cnt)
{
    const int tpb = blockDim.x;
    for (int h = threadIdx.x; h < cells; h += tpb) { key[h] = COVIS_EMPTY; if (val) val[h] = 0; }
    if (cnt && threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t mask = (uint32_t)cells - 1;
    int n_in = 0, n_skip = 0;
    for (int i = threadIdx.x; i < r.len; i += tpb) {
        const int32_t v = a.slots[r.off + i];
        if ((uint32_t)v >= 0x7fffffffu) continue;
        if (!covis_counts(a, v)) { n_skip++; continue; }
        n_in++;
        uint32_t h = covis_hash(v) & mask;
        while (atomicCAS(&key[h], COVIS_EMPTY, v) != COVIS_EMPTY) h = (h + 1) & mask;      // (at most len <= cells / 2 cells are taken)
        if (val) val[h] = (int32_t)((uint32_t)a.octave[r.off + i] << 24);
    }
    if (cnt && n_in) atomicAdd(&cnt[0], n_in);
    if (cnt && n_skip) atomicAdd(&cnt[1], n_skip);
    __syncthreads();
}

__device__ __forceinline__ int covis_wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// one wave: the pair count of stored record r against the hash
__device__ __forceinline__ int covis_record_weight(const CovisQuery& a, const RecordSlot r, int lane, const int32_t* key, uint32_t mask)
{
    int pairs = 0;
    for (int base = 0; base < r.len; base += 64 * COVIS_UNROLL) {             // (r.len = -1 for a free slot: no trip)
        int32_t v[COVIS_UNROLL];
#pragma unroll
        for (int k = 0; k < COVIS_UNROLL; k++) {
            const int i = base + 64 * k + lane;
            v[k] = i < r.len ? a.slots[r.off + i] : COVIS_EMPTY;
        }
#pragma unroll
        for (int k = 0; k < COVIS_UNROLL; k++) {
            if ((uint32_t)v[k] >= 0x7fffffffu) continue;
            uint32_t h = covis_hash(v[k]) & mask;
            for (int32_t c = key[h]; c != COVIS_EMPTY; c = key[h]) { pairs += c == v[k]; h = (h + 1) & mask; }
        }
    }
    return covis_wave_sum(pairs);
}

__device__ __forceinline__ void covis_weights_chunk(const CovisQuery& a, const CovisQ q, int chunk, int32_t* row, const int32_t* key)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t mask = (uint32_t)q.cells - 1;
    for (int k = 0; k < COVIS_WAVE_RECORDS; k++) {
        const int s = chunk * COVIS_CHUNK + k * COVIS_WAVES + wave;           // wave-uniform
        if (s >= a.n_slots) break;
        int w = 0;
        if (s != q.slot) w = covis_record_weight(a, a.slot[s], lane, key, mask);
        if (lane == 0) row[s] = w;
    }
}

__global__ __launch_bounds__(COVIS_TPB) void k_covis_weights(CovisQuery a)
{
    const int n_chunks = (a.n_slots + COVIS_CHUNK - 1) / COVIS_CHUNK;
    const int qi = blockIdx.x / n_chunks, chunk = blockIdx.x - qi * n_chunks;
    const CovisQ q = a.q[qi];
    int32_t* row = a.weights + (size_t)qi * a.n_slots;
    if (q.hash >= 0) {                                                        // uniform over the workgroup
        covis_weights_chunk(a, q, chunk, row, a.g_key + q.hash);              // (k_covis_build wrote n_mps and skipped)
        return;
    }
    int32_t* cnt = covis_lds;                                                 // [4]: the keys start 16 bytes in
    int32_t* key = covis_lds + 4;
    covis_build(a, a.slot[q.slot], q.cells, key, nullptr, cnt);
    if (chunk == 0 && threadIdx.x == 0) { a.n_mps[qi] = cnt[0]; a.skipped[qi] = cnt[1]; }
    covis_weights_chunk(a, q, chunk, row, key);
}

// one workgroup per query whose hash lies in global scratch
__global__ __launch_bounds__(COVIS_TPB) void k_covis_build(CovisQuery a)
{
    const int qi = blockIdx.x;
    const CovisQ q = a.q[qi];
    if (q.hash < 0) return;                                                   // uniform over the workgroup
    int32_t* cnt = covis_lds;
    covis_build(a, a.slot[q.slot], q.cells, a.g_key + q.hash, a.g_val + q.hash, cnt);
    if (threadIdx.x == 0) { a.n_mps[qi] = cnt[0]; a.skipped[qi] = cnt[1]; }
}

// a counter as the atomic adds left it: in global scratch the adds happen in L2, so the read goes there too (in LDS it is a plain read)
__device__ __forceinline__ uint32_t covis_cell(const int32_t* p) { return (uint32_t)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The whole workgroup over the records of weight > 0, then the count of the entries whose counter reached th_obs.  cnt: one LDS
// word that is free once every probe is done (the LDS hash lends its first key).
__device__ __forceinline__ void covis_redundancy(const CovisQuery& a, const CovisQ q, int qi, const int32_t* key, int32_t* val, int32_t* cnt)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t mask = (uint32_t)q.cells - 1;
    const int32_t* row = a.weights + (size_t)qi * a.n_slots;
    const int32_t th = a.th_obs;
    const int n_waves = blockDim.x >> 6;
    int seen = 0;                                                             // records of weight > 0 met so far: dealt to the waves in turn
    for (int s0 = 0; s0 < a.n_slots; s0 += 64) {                              // (they cluster around the query's slot: a wave per range of slots would leave one wave with all of them)
        const int sl = s0 + lane;
        unsigned long long todo = __ballot(sl < a.n_slots && row[sl] > 0);    // (the query's own slot and free slots have weight 0)
        for (; todo; todo &= todo - 1, seen++) {
            if (seen % n_waves != wave) continue;                             // wave-uniform
            const int s = s0 + (int)__builtin_ctzll(todo);
            const RecordSlot r = a.slot[s];
            for (int base = 0; base < r.len; base += 64 * COVIS_UNROLL) {
                int32_t v[COVIS_UNROLL];
#pragma unroll
                for (int k = 0; k < COVIS_UNROLL; k++) {
                    const int i = base + 64 * k + lane;
                    v[k] = i < r.len ? a.slots[r.off + i] : COVIS_EMPTY;
                }
#pragma unroll
                for (int k = 0; k < COVIS_UNROLL; k++) {
                    if ((uint32_t)v[k] >= 0x7fffffffu) continue;
                    uint32_t h = covis_hash(v[k]) & mask;
                    int oct = -1;
                    for (int32_t c = key[h]; c != COVIS_EMPTY; c = key[h]) {
                        if (c == v[k]) {
                            if (oct < 0) oct = a.octave[r.off + base + 64 * k + lane];
                            const uint32_t cell = covis_cell(&val[h]);       // (a count read just before another lane's add lets one more through)
                            if (oct <= (int)(cell >> 24) + 1 && (int32_t)(cell & 0xffffffu) < th) atomicAdd(&val[h], 1);
                        }
                        h = (h + 1) & mask;
                    }
                }
            }
        }
    }
    __syncthreads();
    int n = 0;
    for (int h = threadIdx.x; h < q.cells; h += blockDim.x)
        if (key[h] != COVIS_EMPTY && (int32_t)(covis_cell(&val[h]) & 0xffffffu) >= th) n++;
    n = covis_wave_sum(n);
    __syncthreads();                                                          // every key has been read: cnt may be one of them
    if (threadIdx.x == 0) cnt[0] = 0;
    __syncthreads();
    if (lane == 0 && n) atomicAdd(&cnt[0], n);
    __syncthreads();
    if (threadIdx.x == 0) a.n_redundant[qi] = cnt[0];
}

__global__ __launch_bounds__(COVIS_RED_TPB) void k_covis_redundancy(CovisQuery a)
{
    const int qi = blockIdx.x;
    const CovisQ q = a.q[qi];
    if (q.hash >= 0) {                                                        // uniform over the workgroup
        covis_redundancy(a, q, qi, a.g_key + q.hash, a.g_val + q.hash, covis_lds);
        return;
    }
    int32_t* key = covis_lds;                                                 // 8 bytes a cell: 32 KiB at COVIS_LDS_FEATURES
    int32_t* val = key + q.cells;
    covis_build(a, a.slot[q.slot], q.cells, key, val, nullptr);               // (k_covis_weights wrote n_mps and skipped)
    covis_redundancy(a, q, qi, key, val, key);
}

// one wave per job: the features of one record from the old arena to their place in the new one
__global__ __launch_bounds__(COVIS_TPB) void k_covis_move(CovisMove a)
{
    const int j = blockIdx.x * COVIS_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= a.n_jobs) return;
    const RecordMoveJob job = a.job[j];
    for (int i = lane; i < job.len; i += 64) {
        a.dst_slots[job.dst + i] = a.src_slots[job.src + i];
        a.dst_octave[job.dst + i] = a.src_octave[job.src + i];
    }
}

void covis_launch_build(hipStream_t s, const CovisQuery& a)
{
    if (a.n_q <= 0) return;
    hipLaunchKernelGGL(k_covis_build, dim3(a.n_q), dim3(COVIS_TPB), 16, s, a);
}

void covis_launch_weights(hipStream_t s, const CovisQuery& a, int lds_cells)
{
    if (a.n_q <= 0 || a.n_slots <= 0) return;
    const int n_chunks = (a.n_slots + COVIS_CHUNK - 1) / COVIS_CHUNK;
    hipLaunchKernelGGL(k_covis_weights, dim3((unsigned)(n_chunks * a.n_q)), dim3(COVIS_TPB), 16 + (size_t)lds_cells * 4, s, a);
}

void covis_launch_redundancy(hipStream_t s, const CovisQuery& a, int lds_cells)
{
    if (a.n_q <= 0) return;
    hipLaunchKernelGGL(k_covis_redundancy, dim3(a.n_q), dim3(COVIS_RED_TPB), 16 + (size_t)lds_cells * 8 - (lds_cells ? 16 : 0), s, a);
}

void covis_launch_move(hipStream_t s, const CovisMove& a)
{
    if (a.n_jobs <= 0) return;
    hipLaunchKernelGGL(k_covis_move, dim3((a.n_jobs + COVIS_WAVES - 1) / COVIS_WAVES), dim3(COVIS_TPB), 0, s, a);
}
