// kfdb_kernels.hip -- the device side of the KeyFrameDatabase (kfdb_host.cpp): per stored entry, what the inverted-file walk of
// KeyFrameDatabase::DetectLoopCandidates / DetectMapMatchCandidates (src/Database.cpp:72-327) and L1Scoring::score
// (ScoringObject.cpp:23-68) compute for one query BowVector -- the number of common words, the smallest common word and the score.
//
// One wave per slot.  The wave strides over the ENTRY's words, 64 to a chunk and KFDB_UNROLL chunks to a trip, and every lane
// binary-searches its words in the query (staged in LDS up to KFDB_QUERY_LDS_WORDS words).  __ballot of the hits gives the count and, because both vectors are in
// ascending word order, the lanes of the hits in ascending word order.  The score is a sum of doubles whose ORDER is part of its
// definition (common words ascending, as the reference's merge walk adds them): every hit lane computes its own term, and the
// terms are then added one after the other in lane order into one running double that the wave carries across chunks -- a loop
// over the set bits of the ballot, so its length is the number of common words, not the length of the entry; a chunk with many
// hits takes all 64 lanes in a straight line instead (KFDB_DENSE_HITS).
#include "kfdb_types.h"

__device__ __forceinline__ double kfdb_read_lane(double v, int lane)          // lane is wave-uniform
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

#define KFDB_UNROLL 4                      // chunks of 64 entry words a wave searches side by side in one trip
#define KFDB_DENSE_HITS 16                 // hits in a chunk from which the 64-lane straight-line sum beats the loop over the set bits

__device__ __forceinline__ void kfdb_slot(const KfdbQuery& a, int slot, int lane, const int32_t* q_ids, const double* q_vals)
{
    const RecordSlot s = a.slot[slot];
    const int q_n = a.q_n;
    const int top = q_n > 0 ? 1 << (31 - __builtin_clz(q_n)) : 0;             // the largest power of two <= q_n
    int count = 0, first = -1;
    double sum = 0.0;
    for (int base = 0; base < s.len; base += 64 * KFDB_UNROLL) {              // (s.len = -1 for a free slot: no trip)
        int32_t id[KFDB_UNROLL];
        double wi[KFDB_UNROLL];
        int lo[KFDB_UNROLL];
#pragma unroll
        for (int k = 0; k < KFDB_UNROLL; k++) {
            const int i = base + 64 * k + lane;
            id[k] = 0; wi[k] = 0.0; lo[k] = 0;
            if (i < s.len) { id[k] = a.ids[s.off + i]; wi[k] = a.vals[s.off + i]; }
        }
        // lo = the number of query ids below id: a lower bound with the same trip count in every lane and no branch in it, so that
        // the KFDB_UNROLL searches of a lane are independent chains whose LDS reads overlap
        for (int step = top; step > 0; step >>= 1) {
#pragma unroll
            for (int k = 0; k < KFDB_UNROLL; k++) {
                const int idx = lo[k] + step;
                const int32_t v = q_ids[min(idx, q_n) - 1];                   // (step > 0 only when q_n >= 1)
                lo[k] = (idx <= q_n && v < id[k]) ? idx : lo[k];
            }
        }
#pragma unroll
        for (int k = 0; k < KFDB_UNROLL; k++) {                               // chunk after chunk: the order of the sum
            const int at = min(lo[k], max(q_n - 1, 0));
            const bool hit = base + 64 * k + lane < s.len && lo[k] < q_n && q_ids[at] == id[k];
            double term = 0.0;
            if (hit) {
                const double vi = q_vals[at];
                term = (fabs(vi - wi[k]) - fabs(vi)) - fabs(wi[k]);
            }
            unsigned long long hits = __ballot(hit);
            if (hits == 0) continue;
            if (first < 0) first = __builtin_amdgcn_readlane(id[k], (int)__builtin_ctzll(hits));
            const int n_hits = __popcll(hits);
            count += n_hits;
            if (n_hits >= KFDB_DENSE_HITS) {
                // a chunk full of hits (the query's own entry, a revisited place): all 64 lanes in lane order, straight-line.  The
                // lanes without a hit add their +0.0, which leaves every bit of the sum as it is: the sum starts at +0.0 and can
                // never be -0.0 (round-to-nearest gives -0.0 only from -0.0 + -0.0), and s + 0.0 == s for every other s.
#pragma unroll
                for (int b = 0; b < 64; b++) sum += kfdb_read_lane(term, b);
            } else {
                while (hits) {                                                // wave-uniform: every lane carries the same sum
                    sum += kfdb_read_lane(term, (int)__builtin_ctzll(hits));
                    hits &= hits - 1;
                }
            }
        }
    }
    if (lane == 0) {
        a.words[slot] = count;
        a.first_word[slot] = first;
        a.score[slot] = count ? -sum / 2.0 : 0.0;
    }
}

__global__ __launch_bounds__(64 * KFDB_WAVES) void k_kfdb_query(KfdbQuery a)
{
    __shared__ int32_t q_ids[KFDB_QUERY_LDS_WORDS];
    __shared__ double q_vals[KFDB_QUERY_LDS_WORDS];
    const bool staged = a.q_n <= KFDB_QUERY_LDS_WORDS;                        // uniform over the grid
    if (staged) {
        for (int i = threadIdx.x; i < a.q_n; i += 64 * KFDB_WAVES) { q_ids[i] = a.q_ids[i]; q_vals[i] = a.q_vals[i]; }
        __syncthreads();
    }
    const int slot = blockIdx.x * KFDB_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= a.n_slots) return;                                            // (behind the only barrier)
    if (staged) kfdb_slot(a, slot, lane, q_ids, q_vals);
    else kfdb_slot(a, slot, lane, a.q_ids, a.q_vals);
}

// one wave per job: the words of one entry from the old arena to their place in the new one
__global__ __launch_bounds__(64 * KFDB_WAVES) void k_kfdb_move(KfdbMove a)
{
    const int j = blockIdx.x * KFDB_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= a.n_jobs) return;
    const RecordMoveJob job = a.job[j];
    for (int i = lane; i < job.len; i += 64) {
        a.dst_ids[job.dst + i] = a.src_ids[job.src + i];
        a.dst_vals[job.dst + i] = a.src_vals[job.src + i];
    }
}

void kfdb_launch_query(hipStream_t s, const KfdbQuery& a)
{
    if (a.n_slots <= 0) return;
    hipLaunchKernelGGL(k_kfdb_query, dim3((a.n_slots + KFDB_WAVES - 1) / KFDB_WAVES), dim3(64 * KFDB_WAVES), 0, s, a);
}

void kfdb_launch_move(hipStream_t s, const KfdbMove& a)
{
    if (a.n_jobs <= 0) return;
    hipLaunchKernelGGL(k_kfdb_move, dim3((a.n_jobs + KFDB_WAVES - 1) / KFDB_WAVES), dim3(64 * KFDB_WAVES), 0, s, a);
}
