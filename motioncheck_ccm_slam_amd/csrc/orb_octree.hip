// orb_octree.hip -- keypoint selection of the ORB extractor: DistributeOctTree on the FAST candidates of every level (the stages: orb_types.h).
#include <hip/hip_runtime.h>
#include "orb_types.h"
#include "orb_device.h"

// ------------------------------------------------------------------------------------------------
// k_octree: DistributeOctTree (ORBextractor.cpp:707-931), one workgroup of 4 waves per (frame, level): the loops over
// keys are dealt to the threads (see KEY-PARALLEL FORM in the kernel), the list bookkeeping is computed by every wave
// identically (same LDS values written four times) so that all loop control stays uniform across the block.
//
// The reference keeps nodes in a std::list, inserting children with push_front and erasing the
// parent.  Equivalent array form used here: after a pass in which the nodes P_0..P_{m-1} are divided
// in processing order, the new list is   reverse(children in creation order) ++ (old list minus the
// divided nodes).  The keys are not moved (rounds 1-2 kept them grouped by node in a ping-pong scratch array, a stable 4-way
// partition per divided node: DivideNode pushes keys in order, :681-695): every key carries the list position of its node.
// "Full" passes divide every node holding more than one key, in list order (:774-833).  Once
// size + 3*nToExpand > N the reference switches to dividing in descending (size, address) order and
// stops as soon as size >= N (:841-905); equal sizes are ordered by creation (later first), the
// same deterministic replacement for the address order that the oracle documents.
struct OctNodes {
    int* first; int* count;
    short* x0; short* y0; short* x1; short* y1;
    uint8_t* buf;
};
#define OCT_SET_BYTES 20       // per node in one OctNodes set (17 used)
#define OCT_NODE_LDS 72        // total LDS bytes per list slot: 2 sets + cc[4] + ord + cbase + mark + gain

__device__ __forceinline__ OctNodes oct_carve(char* base, int cap)
{
    OctNodes n;
    n.first = reinterpret_cast<int*>(base);              base += 4 * cap;
    n.count = reinterpret_cast<int*>(base);              base += 4 * cap;
    n.x0 = reinterpret_cast<short*>(base);               base += 2 * cap;
    n.y0 = reinterpret_cast<short*>(base);               base += 2 * cap;
    n.x1 = reinterpret_cast<short*>(base);               base += 2 * cap;
    n.y1 = reinterpret_cast<short*>(base);               base += 2 * cap;
    n.buf = reinterpret_cast<uint8_t*>(base);
    return n;
}

template <int V> struct OctInt { static constexpr int value = V; };

__device__ __forceinline__ int key_x(unsigned k) { return (int)(k & 0xFFFu); }
__device__ __forceinline__ int key_y(unsigned k) { return (int)((k >> 12) & 0xFFFu); }

// Orders the LDS and global accesses of the block's 4 waves between phases.
__device__ __forceinline__ void wave_sync_mem()
{
    __threadfence_block();
    __syncthreads();
}

__device__ __forceinline__ int oct_nonempty(const int* cc, int p)
{
    return (cc[4 * p] > 0) + (cc[4 * p + 1] > 0) + (cc[4 * p + 2] > 0) + (cc[4 * p + 3] > 0);
}

// Diagnostic build only (-DOCT_STAMPS, tools/oct_stamps.py): the level-0 workgroup of frame 0 leaves the shader clock at its phase
// boundaries; the shipped kernel contains none of this.
#ifdef OCT_STAMPS
__device__ unsigned long long oct_stamps[64];
__device__ int oct_stamp_n;
#define OCT_STAMP() do { if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) { const int i__ = oct_stamp_n; if (i__ < 64) { oct_stamps[i__] = __builtin_amdgcn_s_memtime(); oct_stamp_n = i__ + 1; } } } while (0)
extern "C" int ccm_debug_oct_stamps(unsigned long long* out, int* n)
{
    if (hipMemcpyFromSymbol(n, HIP_SYMBOL(oct_stamp_n), 4, 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const int zero = 0;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(oct_stamps), 64 * 8, 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(oct_stamp_n), &zero, 4, 0, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
#else
#define OCT_STAMP() do { } while (0)
#endif
#ifndef OCT_LDS_KEYS
#define OCT_LDS_KEYS 2048       // candidates of a (frame, level) up to which the key-parallel form below is used (its keys and their node ids live in LDS)
#endif
#ifndef OCT_GATHER_CELLS
#define OCT_GATHER_CELLS 512    // cells of a level up to which the gather takes its one-trip form (752x480: 336 at level 0, 1241x376: 440)
#endif
#ifndef OCT_WAVES
#define OCT_WAVES 4             // measured: 1 -> 0.22 ms, 2 -> 0.41, 4 -> 0.135, 8 -> 0.23 ms per 256 frames
#endif
// (Round 3 also put the two key buffers into LDS for levels with <= 2048 candidates -- every level of the bench frames -- so that the
//  passes below chain LDS instead of global round trips: 0.1208 ms against 0.1198 for this kernel, no gain; the passes are bound by
//  their barriers and the list bookkeeping every wave repeats, not by where the keys live.  Not kept.)
// (90 registers = 5 workgroups per CU for 2048 workgroups; forcing 6 / 8 with -DOCT_WPE (40 / 96 bytes of spills) measured no gain:
//  step 1.064 / 1.071 / 1.083 ms at 5 / 6 / 8 -- the kernel is the chain inside a workgroup, not the second round of workgroups)
#ifndef OCT_WPE
#define OCT_WPE 5                // 96 registers: five workgroups per CU
#endif
#define OCT_OCC __attribute__((amdgpu_waves_per_eu(OCT_WPE, OCT_WPE)))
__global__ __launch_bounds__(64 * OCT_WAVES) OCT_OCC void k_octree(const OrbGeom g, const OrbCell* __restrict__ cells,
                                               const unsigned* __restrict__ slots, const int* __restrict__ cell_count,
                                               unsigned* keysA, unsigned* keysB,
                                               unsigned* __restrict__ out, int* __restrict__ out_count,
                                               int* __restrict__ status, int reg_keys_on)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    OCT_STAMP();                                             // 0 start
    // blockIdx.y = level: the long-running fine levels are dispatched first
    const int level = blockIdx.y, f = blockIdx.x + g.frame0, lane = lane_id(), wv = threadIdx.x >> 6;
    const OrbLevel& L = g.lv[level];
    const int cap = g.list_cap;                                          // multiple of 16
    OctNodes cur = oct_carve(smem, cap);
    OctNodes nxt = oct_carve(smem + (size_t)cap * OCT_SET_BYTES, cap);
    int* cc = reinterpret_cast<int*>(smem + (size_t)cap * 2 * OCT_SET_BYTES);   // [cap][4] child key counts
    int* ord = cc + 4 * cap;          // processing order -> list position
    int* cbase = ord + cap;           // creation index of the first child of the k-th divided node
    int* mark = cbase + cap;          // 0 = survivor, k+1 = divided as the k-th
    int* gain = mark + cap;           // careful mode: list growth per candidate, in rank order
    int* shared_len = gain + cap;     // (16 bytes kept between the lists and the keys: lkeys stays 16-byte aligned)

    unsigned* kb[2] = { keysA + (long long)f * g.keys_per_frame + L.key_first,
                        keysB + (long long)f * g.keys_per_frame + L.key_first };
    // KEY-PARALLEL FORM (round 3).  The reference moves
    // a divided node's keys into its children's vectors, and until round 3 this kernel did the same: a stable 4-way partition of
    // every divided node's key range, a wave per node -- half of the kernel's time, most lanes idle on nodes of ~10 keys
    // (tools/r03_oct_stamps.sh).  But a key's position inside its node never matters: DivideNode keeps the keys in their original
    // order, and the only thing read from a node's key list besides its length is "the best response, first key wins ties"
    // (:912-928).  So the keys stay where the gather put them, every key carries the list position of its node, and a pass is
    // a loop over KEYS: count the quadrants of the nodes that may be divided (LDS atomics: sums, order-free), and after the list
    // bookkeeping (unchanged: it never looks at keys) move every key's node id to its child's or its survivor's new position.
    // The final choice is an atomic max per node of (response, original order reversed).
    unsigned* lkeys = reinterpret_cast<unsigned*>(shared_len + 4);                     // [OCT_LDS_KEYS]
    unsigned* best = lkeys + OCT_LDS_KEYS;                                               // [cap]
    unsigned short* surv_pos = reinterpret_cast<unsigned short*>(best + cap);          // [cap] new position of a node that is not divided
    const int N = L.quota;
    int* ocount = out_count + (long long)f * g.nlevels + level;

    // ---- gather this level's candidates in cell-major order (= ccm_orb_debug_candidates' order: "first key wins ties" rests on it)
    const int* ccount = cell_count + (long long)f * g.ncells + L.cell_first;
    const unsigned* fslots = slots + (long long)f * g.slots_per_frame;
    const int tid = threadIdx.x;
    const int R = L.roots;
    constexpr int OCT_KPT = OCT_LDS_KEYS / (64 * OCT_WAVES);
    unsigned mykey[OCT_KPT]; int mynode[OCT_KPT];
#pragma unroll
    for (int j = 0; j < OCT_KPT; j++) { mykey[j] = 0u; mynode[j] = 0; }
    if (tid < ORB_MAX_ROOTS) cc[tid] = 0;                    // the roots' sizes, counted below (the gather's barrier comes first)
    // ONE-TRIP FORM (all keys of the level in one global round trip; two dependent trips in all: the cells' counts, then the keys).  Every wave loads the counts of ALL cells of
    // the level at once (OCT_GCH chunks of 64: no round waits behind another's key stores) and scans them on DPP, so every wave knows
    // every cell's first key and the total with no barrier; a wave leaves the offsets of its own chunks (u % OCT_WAVES == wave) in
    // LDS that is idle until the roots are made -- the two node sets: goffs[cell] = first key, gdelta[cell] = slot_first - first key.
    // Then key k = tid + 256 j (mykey[]'s own mapping: straight to registers and lkeys, all of a thread's loads in flight together)
    // finds its cell by a binary search over goffs -- the last cell whose first key is <= k; an empty cell shares its offset with the
    // next one and is never the last -- and its root is counted the moment it arrives.  Taken where the level has at most
    // OCT_GATHER_CELLS cells (and the sets hold them) and at most OCT_LDS_KEYS candidates; any other level, and the test switch
    // reg_keys_on == 0, take the loop below (until this form: every level, 29,500 of the level-0 workgroup's 112,300 cycles).
    constexpr int OCT_GCH = OCT_GATHER_CELLS / 64, OCT_GPW = OCT_GCH / OCT_WAVES;
    static_assert(OCT_GCH % OCT_WAVES == 0 && OCT_GPW >= 1, "every wave leaves the offsets of OCT_GPW chunks");
    int* goffs = reinterpret_cast<int*>(smem);               // [5 * cap]
    int* gdelta = goffs + 5 * cap;                           // [5 * cap]
    int total = 0;
    bool gathered = false;
    if (reg_keys_on && L.ncells <= min(OCT_GATHER_CELLS, 5 * cap)) {
        int cnt[OCT_GCH], sf[OCT_GPW], myoff[OCT_GPW];
#pragma unroll
        for (int u = 0; u < OCT_GCH; u++) {
            const int ci = 64 * u + lane;
            cnt[u] = ci < L.ncells ? ccount[ci] : 0;
        }
#pragma unroll
        for (int v = 0; v < OCT_GPW; v++) {
            const int ci = 64 * (wv + OCT_WAVES * v) + lane;
            sf[v] = ci < L.ncells ? cells[L.cell_first + ci].slot_first : 0;
            myoff[v] = 0;
        }
#pragma unroll
        for (int u = 0; u < OCT_GCH; u++) {
            const int incl = wave_incl_scan(cnt[u]);
            if (u % OCT_WAVES == wv) myoff[u / OCT_WAVES] = total + incl - cnt[u];
            total += wave_last(incl);
        }
        if (total <= OCT_LDS_KEYS) {
#pragma unroll
            for (int v = 0; v < OCT_GPW; v++) {
                const int ci = 64 * (wv + OCT_WAVES * v) + lane;
                if (ci < L.ncells) { goffs[ci] = myoff[v]; gdelta[ci] = sf[v] - myoff[v]; }
            }
            gathered = true;
        } else total = 0;
    }
    for (int base = 0; base < L.ncells && !gathered; base += 64 * OCT_WAVES) {
        int cnt[OCT_WAVES];
#pragma unroll
        for (int u = 0; u < OCT_WAVES; u++) {
            const int ci = base + 64 * u + lane;
            cnt[u] = ci < L.ncells ? ccount[ci] : 0;
        }
        const int myci = base + 64 * wv + lane;
        const int sfirst = myci < L.ncells ? cells[L.cell_first + myci].slot_first : 0;
        int mydst = 0, mycnt = 0;
#pragma unroll
        for (int u = 0; u < OCT_WAVES; u++) {
            const int incl = wave_incl_scan(cnt[u]);
            if (u == wv) { mydst = total + incl - cnt[u]; mycnt = cnt[u]; }
            total += wave_last(incl);
        }
        const unsigned* sp = fslots + sfirst;
        // (eight loads in flight per cell -- a cell of the bench frames holds up to ~20 candidates: with four per trip this loop was
        //  five dependent global round trips, twice: 30,000 of the kernel's 115,000 cycles, tools/r03_oct_stamps.sh; sixteen cost the
        //  registers that keep five workgroups on a CU)
        for (int k = 0; k < mycnt; k += 8) {
            unsigned v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = sp[min(k + u, mycnt - 1)];
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (k + u < mycnt && mydst + k + u < L.key_cap) {
                    kb[0][mydst + k + u] = v[u];
                    if (mydst + k + u < OCT_LDS_KEYS) lkeys[mydst + k + u] = v[u];
                }
        }
    }
    OCT_STAMP();                                             // 1 the cells' key offsets known (the loop: its keys stored)
    if (total > L.key_cap) { if (lane == 0) atomicOr(status, 1); total = L.key_cap; }
    const int n = total;
    if (n == 0 || N <= 0) { if (threadIdx.x == 0) *ocount = 0; return; }
    const bool small = reg_keys_on && n <= OCT_LDS_KEYS;
    wave_sync_mem();
    OCT_STAMP();                                             // 2 offsets (the loop: keys) visible to the block

    // ---- the loops over keys.  Up to OCT_LDS_KEYS candidates: the thread's keys (k = tid + 256 j) and their nodes' list positions
    //      stay in REGISTERS through all passes (unrolled: the LDS reads of a thread's eight keys are independent and in flight
    //      together).  More: the keys are read from kb[0] and the node ids live in kb[1] (thread t only ever touches the ids of its
    //      own keys, so no barrier is needed for them).
    // fn(key, node, k); mode 0: node read, 1: node read and written, 2: node written
    auto for_keys = [&](auto&& fn, int mode) {
        if (small) {
#pragma unroll
            for (int j = 0; j < OCT_KPT; j++) { const int k = tid + 64 * OCT_WAVES * j; if (k < n) fn(mykey[j], mynode[j], k); }
        } else {
            for (int k = tid; k < n; k += 64 * OCT_WAVES) {
                const unsigned key = kb[0][k];
                int node = mode == 2 ? 0 : (int)kb[1][k];
                fn(key, node, k);
                if (mode != 0) kb[1][k] = (unsigned)node;
            }
        }
    };
    // ---- roots (:711-753): every key's root from its x, the roots' sizes by LDS atomics, empty roots dropped (list order = x order)
    auto count_root = [&](unsigned key, int& node, int) {
        int r = (int)((float)key_x(key) / L.hx); r = min(r, R - 1);
        node = r;
        atomicAdd(&cc[r], 1);
    };
    if (gathered) {
        // the keys, one global trip.  The searches of a thread's keys run step by step side by side -- one basic block, no branch: NJ
        // independent LDS reads in flight per step, nine dependent steps in all -- then all its loads are out together.
        auto fetch = [&](auto nj) {
            constexpr int NJ = decltype(nj)::value;
            int pos[NJ];
#pragma unroll
            for (int j = 0; j < NJ; j++) pos[j] = 0;
#pragma unroll
            for (int step = OCT_GATHER_CELLS / 2; step >= 1; step >>= 1) {
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    const int k = tid + 64 * OCT_WAVES * j, t = pos[j] + step;         // (k >= n: some cell, never used)
                    const int first = goffs[min(t, L.ncells - 1)];
                    pos[j] = (t < L.ncells && first <= k) ? t : pos[j];
                }
            }
#pragma unroll
            for (int j = 0; j < NJ; j++) pos[j] = gdelta[pos[j]];
#pragma unroll
            for (int j = 0; j < NJ; j++) { const int k = tid + 64 * OCT_WAVES * j; if (k < n) mykey[j] = fslots[k + pos[j]]; }
            // (a key's root follows from its x the moment it is loaded: no pass of its own over the keys, no barrier of its own)
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const int k = tid + 64 * OCT_WAVES * j;
                if (k < n) { lkeys[k] = mykey[j]; count_root(mykey[j], mynode[j], k); }
            }
        };
        if (n <= 64 * OCT_WAVES * (OCT_KPT / 2)) fetch(OctInt<OCT_KPT / 2>()); else fetch(OctInt<OCT_KPT>());
    } else {
        if (small) {
#pragma unroll
            for (int j = 0; j < OCT_KPT; j++) { const int k = tid + 64 * OCT_WAVES * j; if (k < n) mykey[j] = lkeys[k]; }
        }
        for_keys(count_root, 2);
    }
    wave_sync_mem();                                         // (the offsets are dead from here: the node sets are the node sets again)
    OCT_STAMP();                                             // 3 keys in registers, roots counted
    // every thread numbers the non-empty roots itself -- 4 bits per root: its list position -- and root r writes its own node
    unsigned rpos = 0u;
    int len = 0;
#pragma unroll
    for (int r = 0; r < ORB_MAX_ROOTS; r++)
        if (r < R) { rpos |= (unsigned)len << (4 * r); len += cc[r] > 0; }
    if (tid < R && cc[tid] > 0) {
        const int p = (int)((rpos >> (4 * tid)) & 15u);
        cur.x0[p] = (short)(int)(L.hx * (float)tid);
        cur.x1[p] = (short)(int)(L.hx * (float)(tid + 1));
        cur.y0[p] = 0; cur.y1[p] = (short)L.bh;
        cur.count[p] = cc[tid];
    }
    for_keys([&](unsigned, int& node, int) { node = (int)((rpos >> (4 * node)) & 15u); }, 1);
    wave_sync_mem();

    // ---- refinement passes
    OCT_STAMP();                                             // 4 roots made
    bool finish = false, careful = false;
    int guard = 0;
    const unsigned long long lt = lanemask_lt();
    while (!finish) {
        if (++guard > 512) { if (lane == 0) atomicOr(status, 2); break; }
        const int prev = len;
        // (1) the nodes holding more than one key, in list order: the full passes divide exactly these, in this
        //     order.  Every wave builds the whole list and reads back only what it wrote itself.
        int nc = 0;
        for (int base = 0; base < len; base += 64) {
            const int p = base + lane;
            const bool dv = p < len && cur.count[p] > 1;
            const unsigned long long m = __ballot(dv);
            if (dv) ord[nc + __popcll(m & lt)] = p;
            nc += __popcll(m);
        }
        // (2) how many keys of every such node fall into each of its quadrants (n1..n4 of DivideNode, :684-694)
        for (int i = tid; i < 4 * len; i += 64 * OCT_WAVES) cc[i] = 0;
        __syncthreads();
        for_keys([&](unsigned key, int& node, int) {
            const int p = node;
            if (cur.count[p] > 1) {
                const int csx = cur.x0[p] + (cur.x1[p] - cur.x0[p] + 1) / 2, csy = cur.y0[p] + (cur.y1[p] - cur.y0[p] + 1) / 2;   // x0 + ceil(w/2)  (:652)
                atomicAdd(&cc[4 * p + (key_x(key) < csx ? 0 : 1) + (key_y(key) < csy ? 0 : 2)], 1);
            }
        }, 0);
        wave_sync_mem();
        OCT_STAMP();                                         // pass: quadrants counted
        // (3) the divided nodes in processing order: ord[k] = list position of the k-th
        int nd = nc;
        if (careful) {
            // descending (count, creation): new children sit at the list front in reverse creation
            // order, so "created later" == smaller position
            // (the quadratic rank loop is most of this kernel's instructions: each wave ranks a quarter of the list)
            const int m_c = nc;
            // (eight LDS reads in flight: one per step was 145 cycles a step, 17,500 of the kernel's 115,000 cycles; the counts in
            //  registers read back with v_readlane measured slower still)
            // PACKED FORM: count << 16 | (0xFFFF - position) per node holding more than one key, 0 for the others, written once (by
            // every wave, as the rest of the bookkeeping: no block barrier) into `best`, idle until the final selection.  Larger
            // count first, smaller position first among equals = larger packed key first, so a node's rank is the number of packed
            // keys above its own: a compare and an add with carry per entry, four entries per ds_read_b128 (before: five VALU
            // instructions per entry, one ds_read_b32 each).  Positions < cap < 2^16 (the host's 150 KB check); counts <= n, so the
            // form holds while n < 2^15 -- checked here, where n is known (the host's bound on a level's candidates, key_cap, is the
            // cells' slots: 75,600 for level 0 of 752x480 frames that bring 1,250); a level above that takes the loop below.
            const bool packed = n < (1 << 15);
            if (packed) {
                unsigned* pk = best;
                const int len16 = (len + 15) & ~15;                                    // <= cap: a multiple of 16
                for (int base = 0; base < len16; base += 64) {
                    const int p = base + lane;
                    if (p < len16) {
                        const int c = p < len ? cur.count[p] : 0;
                        pk[p] = c > 1 ? ((unsigned)c << 16) | (0xFFFFu - (unsigned)p) : 0u;
                    }
                }
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_wave_barrier();
                const uint4* pk4 = reinterpret_cast<const uint4*>(pk);
                for (int base = 64 * wv; base < len; base += 64 * OCT_WAVES) {
                    const int p = base + lane;
                    const unsigned mine = p < len ? pk[p] : 0u;
                    if (mine != 0u) {
                        int rank = 0;
                        for (int q0 = 0; q0 < len16; q0 += 16) {
                            uint4 a[4];
#pragma unroll
                            for (int u = 0; u < 4; u++) a[u] = pk4[(q0 >> 2) + u];
#pragma unroll
                            for (int u = 0; u < 4; u++)
                                rank += (a[u].x > mine) + (a[u].y > mine) + (a[u].z > mine) + (a[u].w > mine);
                        }
                        ord[rank] = p;
                        gain[rank] = oct_nonempty(cc, p) - 1;
                    }
                }
            }
            for (int base = 64 * wv; base < len && !packed; base += 64 * OCT_WAVES) {
                const int p = base + lane;
                const int myc = p < len ? cur.count[p] : 0;
                if (myc > 1) {
                    int rank = 0;
                    for (int q0 = 0; q0 < len; q0 += 8) {
                        int cq[8];
#pragma unroll
                        for (int u = 0; u < 8; u++) cq[u] = cur.count[min(q0 + u, len - 1)];
#pragma unroll
                        for (int u = 0; u < 8; u++) {
                            const int q = q0 + u;
                            rank += (q < len && cq[u] > 1 && (cq[u] > myc || (cq[u] == myc && q < p))) ? 1 : 0;
                        }
                    }
                    ord[rank] = p;
                    gain[rank] = oct_nonempty(cc, p) - 1;
                }
            }
            wave_sync_mem();
            // stop after the first node that brings the list to N (:898); otherwise divide all
            int run = len, K = m_c - 1;
            bool found = false;
            for (int base = 0; base < m_c && !found; base += 64) {
                const int k = base + lane;
                const int gn = k < m_c ? gain[k] : 0;
                const int incl = wave_incl_scan(gn);
                const unsigned long long hit = __ballot(k < m_c && run + incl >= N);
                if (hit != 0ull) { K = base + __ffsll((long long)hit) - 1; found = true; }
                run += wave_last(incl);
            }
            nd = m_c > 0 ? K + 1 : 0;
        }
        OCT_STAMP();                                         // pass: order chosen
        // (4) creation index of each divided node's first child; T = children created in this pass
        int T = 0;
        for (int base = 0; base < nd; base += 64) {
            const int k = base + lane;
            const int ne = k < nd ? oct_nonempty(cc, ord[k]) : 0;
            const int incl = wave_incl_scan(ne);
            if (k < nd) cbase[k] = T + incl - ne;
            T += wave_last(incl);
        }
        // every wave writes all of mark, zeros first: after the barrier each word holds its final value
        for (int base = 0; base < len; base += 64) { const int p = base + lane; if (p < len) mark[p] = 0; }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        for (int base = 0; base < nd; base += 64) { const int k = base + lane; if (k < nd) mark[ord[k]] = k + 1; }
        wave_sync_mem();
        // (5) survivors keep their order behind the new children
        int nsurv = 0;
        for (int base = 0; base < len; base += 64) {
            const int p = base + lane;
            const bool sv = p < len && mark[p] == 0;
            const unsigned long long m = __ballot(sv);
            if (sv) {
                const int dest = T + nsurv + __popcll(m & lt);
                if (dest < cap) {
                    nxt.x0[dest] = cur.x0[p]; nxt.y0[dest] = cur.y0[p]; nxt.x1[dest] = cur.x1[p]; nxt.y1[dest] = cur.y1[p];
                    nxt.count[dest] = cur.count[p];
                    surv_pos[p] = (unsigned short)dest;
                }
            }
            nsurv += __popcll(m);
        }
        const int newlen = T + nsurv;
        if (newlen > cap) { if (lane == 0) atomicOr(status, 4); break; }
        // (6) children, pushed to the front one by one: creation index c -> position T-1-c
        int newExpand = 0;
        for (int base = 0; base < nd; base += 64) {
            const int k = base + lane;
            int gt1 = 0;
            if (k < nd) {
                const int p = ord[k];
                const int px0 = cur.x0[p], py0 = cur.y0[p], px1 = cur.x1[p], py1 = cur.y1[p];
                const int sx = px0 + (px1 - px0 + 1) / 2, sy = py0 + (py1 - py0 + 1) / 2;
                int ci = cbase[k];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int c = cc[4 * p + q];
                    if (c > 0) {
                        const int dest = T - 1 - ci;
                        nxt.x0[dest] = (short)((q & 1) ? sx : px0);
                        nxt.x1[dest] = (short)((q & 1) ? px1 : sx);
                        nxt.y0[dest] = (short)((q & 2) ? sy : py0);
                        nxt.y1[dest] = (short)((q & 2) ? py1 : sy);
                        nxt.count[dest] = c;
                        ci++;
                        gt1 += (c > 1);
                    }
                }
            }
            newExpand += wave_sum(gt1);
        }
        wave_sync_mem();
        // (7) every key follows its node: to the survivor's new position, or to the child of its quadrant (children are created in
        //     quadrant order, empty ones skipped: creation index c -> position T - 1 - c)
        for_keys([&](unsigned key, int& node, int) {
            const int p = node;
            const int mk = mark[p];
            if (mk == 0) node = surv_pos[p];
            else {
                const int csx = cur.x0[p] + (cur.x1[p] - cur.x0[p] + 1) / 2, csy = cur.y0[p] + (cur.y1[p] - cur.y0[p] + 1) / 2;
                const int q = (key_x(key) < csx ? 0 : 1) + (key_y(key) < csy ? 0 : 2);
                int ci = cbase[mk - 1];
                if (q > 0) ci += cc[4 * p] > 0;
                if (q > 1) ci += cc[4 * p + 1] > 0;
                if (q > 2) ci += cc[4 * p + 2] > 0;
                node = T - 1 - ci;
            }
        }, 1);
        __syncthreads();                                     // (these reads of the old list against the next pass's writes into it)
        { OctNodes t = cur; cur = nxt; nxt = t; }
        len = newlen;
        OCT_STAMP();                                         // pass: new list built
        // (8) loop control (:837-905)
        if (len >= N || len == prev) finish = true;
        else if (!careful && len + 3 * newExpand > N) careful = true;
    }

    // ---- keep the best response of every node, first key wins ties (:912-928); order = list order:
    //      max of response << 24 | (0xFFFFFF - original index)   (at most 2^24 candidates per level: 4.2 M at the largest image)
    unsigned* o = out + (long long)f * g.out_per_frame + L.out_first;
    for (int p = tid; p < len; p += 64 * OCT_WAVES) best[p] = 0u;
    __syncthreads();
    for_keys([&](unsigned key, int& node, int k) { atomicMax(&best[node], (key & 0xFF000000u) | (0xFFFFFFu - (unsigned)k)); }, 0);
    __syncthreads();
    for (int p = tid; p < len && p < L.out_cap; p += 64 * OCT_WAVES) {
        const unsigned kidx = 0xFFFFFFu - (best[p] & 0xFFFFFFu);
        o[p] = small ? lkeys[kidx] : kb[0][kidx];
    }
    if (tid == 0) *ocount = min(len, L.out_cap);
    OCT_STAMP();                                             // end
}

size_t orb_octree_lds_bytes(int list_cap) { return (size_t)list_cap * OCT_NODE_LDS + 64 + 4 * (size_t)OCT_LDS_KEYS + 8 * (size_t)list_cap; }
void orb_launch_octree(hipStream_t s, const OrbGeom& g_dev, const OrbCell* cells, int nlevels, int nframes, int list_cap,
                       const unsigned* slots, const int* cell_count, unsigned* keysA, unsigned* keysB,
                       unsigned* out, int* out_count, int* status)
{
    static const int key_parallel = !(getenv("CCM_OCT_REG_KEYS") && atoi(getenv("CCM_OCT_REG_KEYS")) == 0);      // 0: keys and node ids in global memory on every level (test switch: the form levels with > OCT_LDS_KEYS candidates take)
    hipLaunchKernelGGL(k_octree, dim3(nframes, nlevels), dim3(64 * OCT_WAVES), orb_octree_lds_bytes(list_cap), s,
                       g_dev, cells, slots, cell_count, keysA, keysB, out, out_count, status, key_parallel);
}
