// orb_fast_cells.hip -- FAST of the ORB extractor in one kernel: score, per-cell threshold choice and 3x3 NMS on bands of cells whose
// scores stay in LDS (the stages: orb_types.h; the two-kernel path of the bands that do not fit: orb_fast_tiles.hip).
#include <hip/hip_runtime.h>
#include "orb_types.h"
#include "orb_device.h"

// ------------------------------------------------------------------------------------------------
// k_fast_cells: k_fast_score + k_cell_nms fused on a band = a run of cells of one cell row.  The band's pixels
// are staged once in LDS, scored in LDS (rejection test -> survivor list -> dense scoring, in row blocks), and
// each cell's threshold choice / 3x3 NMS / ordered compaction runs straight from the LDS score tile: the score
// map never goes to HBM.  Bands of adjacent cell rows overlap by 6 rows, which are scored twice.
// One band per workgroup.  Round 3 built the alternative -- a workgroup loops over 1..8 consecutive bands and requests the next
// band's pixels (8 registers per thread, one branch-free 16-byte global load per chunk) as soon as the current band is scored, so
// that they arrive under the NMS -- and measured it on one box against this kernel (tools/ab_orb.sh): 0.391 ms at 1 band per
// workgroup, 0.410 / 0.421 / 0.424 / 0.436 / 0.448 at 2 / 3 / 4 / 6 / 8, against 0.368.  A round of the loop (the extra barrier, the
// band record and the kernel arguments re-read through scalar loads, 64 registers instead of 54) costs more than a fresh workgroup,
// whose start-up the dispatcher overlaps with the seven others on the CU.  Not kept.
// NMS works on the list of scored pixels (FC_NZ entries) and the list of local maxima (FC_KEPT); a band that overflows
// either list takes the per-cell row scan instead.
// The kernel is bound by the dependent chain of one band (8 bands per CU, each issuing for a tenth of its life).  The first NMS pass
// therefore requests a scored pixel's eight neighbours and its column's cell together, and a cell's count comes from the per-cell
// counters, not from a scan of its bucket by the last wave (0.367 -> 0.354 ms with the global-address-space staging loads).
// Measured and dropped (profiles/fc_chain_ab.txt): the rank loop reading its bucket eight entries per wait (nothing), all staging
// trips of a thread in flight before the first store (+0.002 ms), the next rejection run's LDS dwords requested before the current
// run's ballots (+0.012 ms, 60 registers), the column masks requested with the pixel dwords (nothing).
// The rejection test takes its items -- one dword = four pixels each -- from the dwords dw_lo .. dw_hi that hold detection columns, not
// from every dword of the tile (3791 runs of 64 per 752x480 frame against 4292; the dominant 4-cell band 16 runs dealt 4 / 4 / 4 / 4
// to the waves, not 18 dealt 5 / 5 / 4 / 4), by fc_item_* of orb_device.h, which the host runs too (ccm_debug_fc_items).  A run is 71
// vector instructions (80 before: profiles/fc_reject_static.txt): run number and stack count in scalar registers, west / east pixels
// by one v_perm_b32 each, the wave's last run drains its stack itself.  0.328 -> 0.3125 ms (profiles/fc_reject_ab.txt).
// The head: ONE scalar wait in front of the pixel loads.  There were four, each dependent on the one before (the status-word pointer,
// tested at the top; the work-order switch and the pointer block, 2.5 KB into the arguments behind OrbGeom by value; the OrbGeom fields
// with half of the band record; the other half behind 130 instructions of exec-mask branching on wave 0), 4,600 of a band's
// 24,500 cycles.  Now the arguments the head needs come first and the rest is 40 bytes (FcLate), the band record is fetched whole in
// one batch with FcLate, a thread's first 16-byte chunk is requested, and the status clear, the counters' zeroing and the NMS's tables
// (by the last wave, from vector loads of its own) run under that trip.  0.3125 -> 0.298 ms; with the kernel-argument preload
// (csrc/Makefile) 0.297, apart from 0.298 in every round at 200 and at 400 steps (profiles/fe_prelude_ab.txt); wave 0's "band record
// arrived -> pixel loads can be issued" 2,640 -> 772 cycles (profiles/fe_prelude_stamps.txt).  Whether the firmware preloads the stamps
// do not show: "start -> band record arrived" is the record's own trip, 912 / 892 / 928 cycles (parent / without / with the flag).
// Looked at on the assembly and dropped: the scalar-register pins of the band's cells behind the pixel loads too (the demand passes
// the 80 scalar registers of eight waves per SIMD; the spills wait on their own loads in front of the pixel loads).
// The NMS's first pass: THREE LDS trips per iteration, not five (profiles/fc_nms_static.txt).  The count of scored pixels and the thread's
// first list entry are one batch (pinned: the compiler moves the entry's read behind the test of the count); the colcell byte carries
// "left / right neighbour inside the cell's rectangle", so the cell's first column and width are not read; a `kept` entry packs the
// tile column, so the second pass does not read the first column either and takes a cell's slots in one 8-byte read; row = pos / pitch
// by the band record's reciprocal and the bucket capacity by selects -- two integer divisions stood between the list's read and the
// neighbours'.  0.2965-0.2973 -> 0.2948-0.2960 ms, apart in the kernel's own time, not in the step (profiles/fc_nms_ab.txt).
// Measured and dropped there: the second pass with A WAVE PER CELL (cell_k, cell_hi and the wave's bucket, one entry per lane, in one batch
// of reads; the slots from the scalar pins; the rank of a bucket of up to 64 from v_readlane, no LDS access in the loop).  Its tail is
// shorter on the stamps (wave 0's "local maxima -> written" 2,372 -> 1,908 cycles) and the kernel is SLOWER: 0.3176-0.3182 ms with a
// rank loop of 11 instructions per entry, 0.3086-0.3093 with 5, 0.3067-0.3076 with the slots from the LDS table (the eight pins live
// across the kernel cost 5 scalar registers more).  Every phase of the band got longer, the untouched rejection + scoring too (9,664 ->
// 10,276 cycles): four waves now run the tail's address arithmetic and a rank loop over their own cell where one wave ranked all cells
// lane-parallel in max(bucket) rounds and three waves left; those instructions are issued beside the seven other bands of the CU.
#ifndef FC_NZ
#define FC_NZ 1024
#endif
#ifndef FC_KEPT
#define FC_KEPT 480             // + the per-cell bucket counters = the 20480 bytes of LDS that let 8 workgroups share a CU on the 4-cell bands
#endif
#define FC_CELLS 32
#ifndef FC_TPB
#define FC_TPB 256              // threads per band workgroup (measured: 192 0.56, 256 0.52, 320 0.75, 384 0.82 ms)
#endif
static_assert(FC_TPB == FC_ITEM_STRIDE, "the band record carries the item steps of FC_WAVES waves (fc_enum, orb_device.h)");
// Survivors of the rejection test wait on the wave's own stack in LDS (running count in a scalar register, no atomic) and are scored
// 64 at a time: the stack never holds more than 63 waiting entries + the 256 pixels of one run of 64 four-pixel items.
#define FC_WAVE_CAP 320         // wave-local stack: at most 63 waiting + the 256 pixels of one item
__host__ __device__ inline size_t fc_lds_bytes(int pitch, int bh)
{
    return 2 * (size_t)pitch * bh + (size_t)FC_WAVE_CAP * (FC_TPB / 64) * 2 + 32 + FC_NZ * 2 + FC_KEPT * 4 + FC_CELLS * 16 + 64 * 8 + 256 + 64;
}

// The rejection test runs on two pixels per register with the packed 16-bit VALU (v_pk_sub_u16 / v_pk_max_u16 /
// v_pk_min_u16): |v - n| <= t  <=>  (u16)(v + t - n) <= 2t.
__device__ __forceinline__ unsigned fc_u(fc_us2 x) { return __builtin_bit_cast(unsigned, x); }      // (fc_pk: orb_device.h)
__device__ __forceinline__ int fc_mbcnt(unsigned long long m, int base)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, (unsigned)base));
}
// Diagnostic build only (-DFC_STAMPS, tools/fc_stamps.py): wave 0 (slots 0-7) and the last wave (slots 8-15) of every workgroup leave the shader clock at their phase
// boundaries in a buffer no other code reads; the shipped kernel contains none of this.
#ifdef FC_STAMPS
#define FC_STAMP_SLOTS 16
#define FC_STAMP_WGS (1 << 17)
__device__ unsigned long long fc_stamps[FC_STAMP_WGS * FC_STAMP_SLOTS];
#define FC_STAMP(k) do { if (threadIdx.x == 0 || threadIdx.x == FC_TPB - 1) { const unsigned wg__ = blockIdx.y * gridDim.x + blockIdx.x; if (wg__ < FC_STAMP_WGS) fc_stamps[wg__ * FC_STAMP_SLOTS + (threadIdx.x ? 8 : 0) + (k)] = __builtin_amdgcn_s_memtime(); } } while (0)
extern "C" int ccm_debug_fc_stamps(unsigned long long* out, int n_wgs)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fc_stamps), (size_t)n_wgs * FC_STAMP_SLOTS * 8, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#else
#define FC_STAMP(k) do { } while (0)
#endif
// image pixels in the global address space (global_load_*, not flat_load_*); fc_u32x4_a4: 16 bytes at a 4-byte-aligned address
typedef const __attribute__((address_space(1))) uint8_t fc_gbyte;
typedef const __attribute__((address_space(1))) unsigned fc_gu32;
typedef const __attribute__((address_space(3))) uint8_t fc_lbyte;      // a byte of LDS by its 32-bit address
typedef unsigned fc_u32x4 __attribute__((ext_vector_type(4)));
typedef fc_u32x4 fc_u32x4_a4 __attribute__((aligned(4)));
// Argument order: everything that stands in front of the pixel loads comes first -- the band table, the work-order switch and the grid
// sizes it needs (explicit: gridDim is a load from the hidden arguments, behind everything else), the call's first frame and level 0's
// image (the caller's: per call) -- 11 dwords, which arrive in scalar registers with the wave where the firmware preloads kernel
// arguments (csrc/Makefile) and in one scalar load where it does not.  The band record's loads are then the kernel's first or second
// batch, and the only wait in front of the pixel loads is theirs.  What is used behind them follows as FcLate: the few fields of
// OrbGeom that the kernel reads (the geometry itself, 2.5 KB by value, stood FIRST until the head was cut: every pointer the head
// needs 2.5 KB into the argument block, no preload possible), the outputs and the status word.
struct FcLate {
    int ini_th, min_th, ncells, slots_per_frame;      // of OrbGeom
    const OrbCell* cells; unsigned* slots; int* cell_count;
    int* clear_status;                                // the extractor's status word where this launch opens a call, else nullptr
};
__global__ __launch_bounds__(FC_TPB) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_fast_cells(const OrbBand* __restrict__ bands, int xcd_on, unsigned grid_x, unsigned grid_y, int frame0,
                                                    const uint8_t* __restrict__ img0, long long plane0, int pitch0, const FcLate g)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fc_smem[];
    int wx, wy;
    xcd_work_item(xcd_on, grid_x, grid_y, wx, wy);
    FC_STAMP(0);
    const OrbBand B = bands[wx];
#ifdef FC_STAMPS
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // (diagnostic: the band descriptor has arrived)
#endif
    FC_STAMP(6);
    // the band's cells, held in scalar registers from here on (left to itself the compiler loads them again where the NMS uses them:
    // another scalar-load latency in each of its two passes, +1,400 cycles per band measured).  The pins also make the compiler fetch
    // the WHOLE record here, in one batch with one wait: it used to leave four of the eight loads behind the first wait, and a field
    // that is not pinned (the reciprocals, before they were) gets a scalar load and a wait of its own on the staging path.  They cost
    // a dozen scalar instructions in front of the pixel loads; moved behind them they raised the scalar-register demand past the 80
    // that eight waves per SIMD allow, and the spills put waits of their own in front of the loads.
    int bclo[4], bcwd[4], bsfirst[4], bscap[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        bclo[i] = B.clo[i]; bcwd[i] = B.cwd[i]; bsfirst[i] = B.slot_first[i]; bscap[i] = B.slot_cap[i];
        asm volatile("" : "+s"(bclo[i]), "+s"(bcwd[i]), "+s"(bsfirst[i]), "+s"(bscap[i]));
    }
    int bxa = B.xa, by0 = B.y0, bncells = B.ncells, bcfirst = B.cell_first;
    asm volatile("" : "+s"(bxa), "+s"(by0), "+s"(bncells), "+s"(bcfirst));
    // i / PW and i / PQ by multiply-shift: exact for i < 2^20 / PW (i <= 65 * 64 here)
    unsigned pw_inv = B.pw_inv, pq_inv = B.pq_inv;
    asm volatile("" : "+s"(pw_inv), "+s"(pq_inv));
    const int f = wy + frame0, tid = threadIdx.x, lane = lane_id(), wv = tid >> 6;
    // the level's image: from the band record, except level 0 (the caller's frames: pointer, pitch and plane are per call and sit at a
    // fixed place at the front of the kernel arguments -- no load that depends on the band record)
    const bool lvl0 = B.level == 0;
    const uint8_t* const Limg = lvl0 ? img0 : B.img;
    const long long Lplane = lvl0 ? plane0 : B.plane;
    const int Lpitch = lvl0 ? pitch0 : B.lpitch, Lw = B.w, Lh = B.h;
    const int P = B.pitch, bh = B.bh, PW = P >> 2;
    uint8_t* T = fc_smem;                                   // pixels  [bh][P]
    uint8_t* S = fc_smem + (size_t)P * bh;                  // scores  [bh][P]
    constexpr int NW = FC_TPB / 64;
    const int WCAP = FC_WAVE_CAP;
    unsigned short* surv = reinterpret_cast<unsigned short*>(S + (size_t)P * bh);     // [NW][WCAP]
    int* nsurv = reinterpret_cast<int*>(surv + NW * WCAP);   // [1] scored pixels, [2] local maxima, [4 + w] survivors of wave w in the row block
    unsigned short* nz = reinterpret_cast<unsigned short*>(nsurv + 8);
    unsigned* kept = reinterpret_cast<unsigned*>(nz + FC_NZ);
    int* cell_hi = reinterpret_cast<int*>(kept + FC_KEPT);   // per cell: local maxima with score >= iniThFAST
    int* cell_n = cell_hi + FC_CELLS;                        // per cell: keypoints written
    int* cell_k = cell_n + FC_CELLS;                         // per cell: local maxima in the cell's bucket of `kept`
    uint2* colmask = reinterpret_cast<uint2*>(cell_k + FC_CELLS + FC_CELLS);     // per tile dword: 16-bit lane masks of its detection columns: .x pixels 0 and 2, .y pixels 1 and 3
    // (what the NMS needs of a cell -- its detection columns and its candidate slots -- comes with the band record: until round 3 the
    //  cell records were loaded from global memory, first on the NMS's critical path, then in front of the pixel loads)
    // [256] per tile column: its cell (bits 0-1), "has a left neighbour inside the cell's rectangle" (bit 2), "has a right one" (bit 3);
    // 255 = no cell's detection column (a cell's byte is <= 15)
    uint8_t* colcell = reinterpret_cast<uint8_t*>(colmask + 64);
    // per cell, for the NMS's second pass: first candidate slot and number of slots, one 8-byte read (indexed per lane there: an LDS read
    // measured 0.7 % faster than three selects on the scalar registers).  The cell's first column and width stood here too until the
    // colcell byte took the edge flags and a `kept` entry the tile column.
    int2* l_slot = reinterpret_cast<int2*>(colcell + 256);
    // (the counters and this table are written behind the pixel loads, by the last wave: see there)
    const OrbBand* const brec = bands + wx;
    const uint8_t* img = Limg + (long long)f * Lplane;
    // ---- stage pixels (clamped: duplicates are only read for pixels whose score is not needed), zero the scores
    const bool dword_ok = ((reinterpret_cast<uintptr_t>(img) | (uintptr_t)Lpitch) & 3) == 0 && Lpitch >= ((Lw + 3) & ~3);
#ifdef FC_STAMPS
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // (diagnostic: level record and everything scalar before the pixel loads has arrived)
#endif
    FC_STAMP(5);
    // the image is read through global-address-space pointers: `img` is a select between a kernel argument and a field of the band
    // record, and left generic its loads become flat_load_dword, four per 16-byte chunk
    fc_gbyte* const gimg = (fc_gbyte*)img;
    // ---- What the pixel addresses do not need runs under the pixel loads' trip: under_trip() stands between a thread's first load and
    // the store of what it returns on the 16-byte path, behind the loop on the two others.
    auto under_trip = [&]() {
        // The status word: zeroed by the first thread of the launch that opens a call (a one-level pyramid starts here; nullptr
        // otherwise).  This kernel never ORs into the word, and stream order still puts the store before every kernel that does.
        if (g.clear_status && (blockIdx.x | blockIdx.y | threadIdx.x) == 0) *g.clear_status = 0;
        // The NMS counters and its per-cell slot table, by the LAST wave (one staging trip on the dominant band where wave 0 has two): lane
        // FC_TPB - 1 - k writes entry k, and takes its table entry from the band record by vector loads of its own.  (Until the head
        // was cut, three blocks `if (tid < ..)` on wave 0 IN FRONT of its pixel loads, the table entries picked from the scalar
        // registers by three selects each: about 100 instructions of exec-mask branching on the path to the loads.)
        const int k = FC_TPB - 1 - tid;
        if (k < FC_CELLS) {
            cell_hi[k] = 0; cell_n[k] = 0; cell_k[k] = 0;
            if (k < 2) nsurv[1 + k] = 0;
            if (k < ORB_BAND_CELLS) l_slot[k] = make_int2(brec->slot_first[k], brec->slot_cap[k]);
        }
    };
    if (dword_ok && (P & 15) == 0) {
        // 16 bytes per lane: one global_load_dwordx4 and two ds_write_b128 (pixels, zeroed scores) per 16 pixels; the last
        // chunks of a row are clamped dword by dword (four global_load_dword)
        const int wmax = ((Lw - 1) & ~3);
        const int PQ = P >> 4, nq = bh * PQ;
        auto chunk = [&](int i) {
            const int ly = (int)(((unsigned)i * pq_inv) >> 20), lq = i - ly * PQ;
            const int gy = min(B.y0 + ly, Lh - 1), gx = B.xa + 16 * lq;
            fc_gbyte* rowp = gimg + (long long)gy * Lpitch;
            fc_u32x4 v;
            if (gx + 12 <= wmax) v = *reinterpret_cast<const __attribute__((address_space(1))) fc_u32x4_a4*>(rowp + gx);
            else {
                v.x = *reinterpret_cast<fc_gu32*>(rowp + min(gx, wmax));
                v.y = *reinterpret_cast<fc_gu32*>(rowp + min(gx + 4, wmax));
                v.z = *reinterpret_cast<fc_gu32*>(rowp + min(gx + 8, wmax));
                v.w = *reinterpret_cast<fc_gu32*>(rowp + min(gx + 12, wmax));
            }
            return v;
        };
        // the thread's first chunk is requested, the set-up runs, and only then is the chunk waited for and stored
        fc_u32x4 v0 = { 0u, 0u, 0u, 0u };
        if (tid < nq) v0 = chunk(tid);
        asm volatile("" ::: "memory");                             // (the request stays in front of the set-up's stores)
        under_trip();
        if (tid < nq) {
            reinterpret_cast<fc_u32x4*>(T)[tid] = v0;
            reinterpret_cast<uint4*>(S)[tid] = make_uint4(0u, 0u, 0u, 0u);
        }
        for (int i = tid + FC_TPB; i < nq; i += FC_TPB) {
            const fc_u32x4 v = chunk(i);
            reinterpret_cast<fc_u32x4*>(T)[i] = v;
            reinterpret_cast<uint4*>(S)[i] = make_uint4(0u, 0u, 0u, 0u);
        }
    } else if (dword_ok) {
        const int wmax = ((Lw - 1) & ~3);
        for (int i = tid; i < bh * PW; i += FC_TPB) {
            const int ly = (int)(((unsigned)i * pw_inv) >> 20), lx = i - ly * PW;
            const int gy = min(B.y0 + ly, Lh - 1), gx = min(B.xa + 4 * lx, wmax);
            reinterpret_cast<unsigned*>(T)[i] = *reinterpret_cast<fc_gu32*>(gimg + (long long)gy * Lpitch + gx);
            reinterpret_cast<unsigned*>(S)[i] = 0u;
        }
        under_trip();
    } else {
        for (int i = tid; i < bh * P; i += FC_TPB) {
            const int ly = i / P, lx = i - ly * P;
            const int gy = min(B.y0 + ly, Lh - 1), gx = min(B.xa + lx, Lw - 1);
            T[i] = gimg[(long long)gy * Lpitch + gx];
            S[i] = 0;
        }
        under_trip();
    }
#ifdef FC_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // (diagnostic: this wave's pixels have arrived)
#endif
    FC_STAMP(7);
    // columns of the tile that belong to some cell's detection area: [c_lo, c_hi)
    const int c_lo = B.c_lo, c_hi = B.c_hi;
    const int t_lo = min(g.ini_th, g.min_th);
    // first of the dwords that hold at least one detection column and have both neighbours inside the row (B.items.n_dw of them)
    const int dw_lo = B.dw_lo;
    if (tid < PW) {
        unsigned mk[4];
        for (int i = 0; i < 4; i++) mk[i] = (4 * tid + i >= c_lo && 4 * tid + i < c_hi) ? 0xFFFFu : 0u;
        colmask[tid] = make_uint2(mk[0] | (mk[2] << 16), mk[1] | (mk[3] << 16));
    }
    __syncthreads();
    FC_STAMP(1);
    if (tid < P) {                                           // (read after the next barrier)
        int ci = 255, lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < ORB_BAND_CELLS; i++) {
            const bool in = i < bncells && tid >= bclo[i] && tid < bclo[i] + bcwd[i];
            ci = in ? i : ci; lo = in ? bclo[i] : lo; hi = in ? bclo[i] + bcwd[i] : hi;
        }
        // xx = tid - lo: a left neighbour where xx > 0, a right one where xx + 1 < cwd (both 0 outside the cells: 255 stays 255)
        colcell[tid] = (uint8_t)(ci | (tid > lo && tid < hi ? 4 : 0) | (tid + 1 < hi ? 8 : 0));
    }
    const int wvs = __builtin_amdgcn_readfirstlane(wv);        // the wave's number in a scalar register: its stack's address and its runs are scalar
    unsigned short* wsurv = surv + wvs * WCAP;
    // ---- rejection + scoring, WAVE-LOCAL (round 3): a wave tests its own runs of 64 items (4 pixels per lane), pushes the survivors on
    // its own stack in LDS, and scores them 64 at a time -- a full wave per scoring pass (97 vector instructions) -- as soon as 64 are waiting.  No
    // workgroup barrier until every pixel of the band is scored: round 2 pooled the survivors of a row block over the four waves
    // (two barriers per row block, and every wave waited for the slowest at each of them).  The stack never holds more than
    // 63 + 256 entries.  The order in which pixels are scored does not matter: the NMS below works on the set.
    //
    // Scoring, ONE POLARITY PER PASS.  A stack entry is the pixel's tile offset (< 2^15: the host keeps pitch * bh below that) and, in
    // bit 15, "the darker polarity only".  A pass pops up to 64 entries and scores each in the polarity its four compass pixels allow
    // (fast_arc16_split, orb_device.h, with the lemma: a polarity whose compass flag is false scores below t_lo and cannot change
    // what is stored); a pixel with neither flag stores nothing.  Where both flags hold (0.1 % of the survivors on level 0, 2-6 % above)
    // the brighter polarity is scored now and the entry goes back on the stack with bit 15 set; such an entry is scored in the darker
    // polarity and never pushed again.  At most one of the two passes stores (a stored score > 0 needs 9 ring pixels strictly
    // brighter than v, or 9 strictly darker, and the ring has 16), so S[pos] and the `nz` list need no maximum and no second entry.
    // Stack bound: a pass pops n = min(wcnt, 64) entries and pushes back at most n, so the stack never grows while it is drained, and
    // it is drained below 64 before the next run of items pushes at most 256: FC_WAVE_CAP holds as before.  The drain ends: every
    // pass either pops an unflagged entry for good or, holding flagged entries only, pushes nothing.
    // The ring is read from seven row bases with the column 0..6 in the ds_read_u8 offset field (the row offsets k * P are
    // run-time values: left to itself the compiler builds sixteen addresses).
    const unsigned t_lds = (unsigned)(uintptr_t)(fc_lbyte*)T;   // the tile's LDS address: the row bases are LDS addresses, not offsets into T
    const int thr = max(t_lo, 1);                              // score >= t_lo && score > 0  <=>  arc = score + 1 > max(t_lo, 1)
    int wcnt = 0;                                              // entries on this wave's stack (wave-uniform)
    auto score_top = [&]() {
        wcnt = __builtin_amdgcn_readfirstlane(wcnt);           // (wave-uniform by construction; this keeps the stack arithmetic scalar)
        const int n = min(wcnt, 64);
        wcnt -= n;
        const bool on = lane < n;
        const unsigned long long on_mask = n >= 64 ? ~0ull : (1ull << n) - 1ull;
        const unsigned popped = wsurv[wcnt + lane];            // (in bounds for every lane: wcnt + 63 < FC_WAVE_CAP)
        const unsigned ent = on ? popped : (unsigned)(3 * P + 3);
        const int pos = (int)(ent & 0x7FFFu);
        int rb[7];
#pragma unroll
        for (int k = 0; k < 7; k++) rb[k] = pos + (int)(t_lds + (unsigned)((k - 3) * P - 3));
#define FC_PX(dx, dy) (*(fc_lbyte*)(uintptr_t)(unsigned)(rb[(dy) + 3] + ((dx) + 3)))
        const int v = FC_PX(0, 0);
        int r[16];
        r[0] = FC_PX(0, 3);    r[1] = FC_PX(1, 3);    r[2] = FC_PX(2, 2);    r[3] = FC_PX(3, 1);
        r[4] = FC_PX(3, 0);    r[5] = FC_PX(3, -1);   r[6] = FC_PX(2, -2);   r[7] = FC_PX(1, -3);
        r[8] = FC_PX(0, -3);   r[9] = FC_PX(-1, -3);  r[10] = FC_PX(-2, -2); r[11] = FC_PX(-3, -1);
        r[12] = FC_PX(-3, 0);  r[13] = FC_PX(-3, 1);  r[14] = FC_PX(-2, 2);  r[15] = FC_PX(-1, 3);
#undef FC_PX
        auto store = [&](bool st, int arc) {
            if (st) {
                S[pos] = (uint8_t)(arc - 1);
                const int q = atomicAdd(nsurv + 1, 1);
                if (q < FC_NZ) nz[q] = (unsigned short)pos;
            }
        };
        if (t_lo < 0) {                                        // (no rejection by the compass pixels below 0: the full score)
            const int arc = fast_score16(v, r) + 1;
            store(on && arc > thr, arc);
            return;
        }
        bool again;
        const int arc = fast_arc16_split(v, r, t_lo, (ent >> 15) != 0u, &again);
        store(on && arc > thr, arc);
        const unsigned long long mb = __ballot(again) & on_mask;
        if (mb != 0ull) {
            if (on && again) wsurv[fc_mbcnt(mb, wcnt)] = (unsigned short)(ent | 0x8000u);
            wcnt += __popcll(mb);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        }
    };
    {
        // the items: the dwords dw_lo .. dw_hi of rows 3 .. bh - 4, run R of 64 to wave R % FC_WAVES (fc_item_*, orb_device.h)
        const int n_dw = B.items.n_dw, d_step = B.items.d_step, r_step = B.items.r_step;
        const int runs = fc_item_runs(bh, n_dw), dw_end = dw_lo + n_dw;
        FcItem item = fc_item_start(dw_lo, n_dw, B.items.nd_inv, wv, lane);
        // `run` and the stack count are wave-uniform and kept in scalar registers: the bases of the v_mbcnt pairs, the sums of the
        // ballots' bit counts and the two loop tests are scalar instructions
        for (int run = wvs; run < runs; run += FC_WAVES) {
            wcnt = __builtin_amdgcn_readfirstlane(wcnt);
            const int pos0 = fc_item_pos0(item, P);             // the item: pixels pos0 .. pos0 + 3 of the tile
            unsigned kk0 = 0, kk1 = 0;                          // 16-bit halves, .lo/.hi of kk0 = pixels 0 / 2, of kk1 = pixels 1 / 3
            if (fc_item_valid(item, bh)) {
                const unsigned* crow = reinterpret_cast<const unsigned*>(T + pos0);
                const unsigned c0 = crow[-1], c1 = crow[0], c2 = crow[1];
                const unsigned nn = crow[3 * PW], ss = crow[-3 * PW];
                const fc_us2 tt = fc_pk((unsigned)t_lo * 0x00010001u);
                unsigned kk[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {                                     // h = 0: pixels 0 and 2; h = 1: pixels 1 and 3
                    const unsigned sel = h ? 0x0c030c01u : 0x0c020c00u;           // v_perm_b32: two bytes -> two u16
                    const fc_us2 v = fc_pk(__builtin_amdgcn_perm(0u, c1, sel));
                    const fc_us2 n = fc_pk(__builtin_amdgcn_perm(0u, nn, sel)), sq = fc_pk(__builtin_amdgcn_perm(0u, ss, sel));
                    // west = columns px - 3 + i, east = px + 3 + i of pixel i: bytes 1, 3 (h = 1: 2, 4) of c0:c1 and 3, 5 (4, 6) of c1:c2,
                    // one v_perm_b32 over the dword pair each
                    const fc_us2 w = fc_pk(__builtin_amdgcn_perm(c1, c0, h ? 0x0c040c02u : 0x0c030c01u));
                    const fc_us2 e = fc_pk(__builtin_amdgcn_perm(c2, c1, h ? 0x0c060c04u : 0x0c050c03u));
                    // every 9-arc holds ring pixel k or k+8: a corner brighter (darker) than v by more than t needs the
                    // larger (smaller) of BOTH opposite pairs beyond v + t (v - t)
                    const fc_us2 bm = __builtin_elementwise_min(__builtin_elementwise_max(n, sq), __builtin_elementwise_max(e, w));
                    const fc_us2 dm = __builtin_elementwise_max(__builtin_elementwise_min(n, sq), __builtin_elementwise_min(e, w));
                    kk[h] = fc_u(__builtin_elementwise_sub_sat(bm, (fc_us2)(v + tt))) | fc_u(__builtin_elementwise_sub_sat(__builtin_elementwise_sub_sat(v, tt), dm));
                }
                const uint2 cm = colmask[item.dw];
                kk0 = kk[0] & cm.x; kk1 = kk[1] & cm.y;
            }
            fc_item_step(item, dw_end, n_dw, d_step, r_step);
            // survivor predicates of the lane's four pixels: one 16-bit compare each
            const bool k0 = (kk0 & 0xFFFFu) != 0u, k1 = (kk1 & 0xFFFFu) != 0u;
            const bool k2 = (kk0 >> 16) != 0u, k3 = (kk1 >> 16) != 0u;
            const unsigned long long m0 = __ballot(k0), m1 = __ballot(k1), m2 = __ballot(k2), m3 = __ballot(k3);
            if ((m0 | m1 | m2 | m3) != 0ull) {
                // stack slot of the lane's pixel i among the wave's survivors of this item: pixels 0 of all lanes first, then
                // pixels 1, ...; v_mbcnt counts the lower lanes, and the running base goes into the scalar part of the address
                const int b1 = wcnt + __popcll(m0), b2 = b1 + __popcll(m1), b3 = b2 + __popcll(m2);
                if (k0) (wsurv + wcnt)[fc_mbcnt(m0, 0)] = (unsigned short)pos0;
                if (k1) (wsurv + b1)[fc_mbcnt(m1, 0)] = (unsigned short)(pos0 + 1);
                if (k2) (wsurv + b2)[fc_mbcnt(m2, 0)] = (unsigned short)(pos0 + 2);
                if (k3) (wsurv + b3)[fc_mbcnt(m3, 0)] = (unsigned short)(pos0 + 3);
                wcnt = b3 + __popcll(m3);
                // the LDS operations of one wave complete in order; the fence keeps the compiler from moving the pops above the pushes
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            }
            // scored 64 at a time while another run follows; the wave's last run empties the stack
            const int leave = run + FC_WAVES < runs ? 63 : 0;
            while (wcnt > leave) score_top();
        }
    }
    __syncthreads();
    FC_STAMP(2);
    // ---- NMS on the list of scored pixels.  With minThFAST <= iniThFAST every stored score is >= minThFAST, so
    // "keep at threshold th" == score >= th and strictly greater than every neighbour inside the cell's rectangle.
    // The count of scored pixels and the thread's first list entry are requested together: nz[tid] is inside the list for every thread
    // and is used only where tid < nnz.
    static_assert(FC_TPB <= FC_NZ, "nz[tid] is read before nnz is known");
    const int nnz = nsurv[1];
    int nz0 = nz[tid];
    asm volatile("" : "+v"(nz0));                            // (left to itself the compiler moves the read behind the test of nnz: a trip of its own)
    const int rh = bh - 6;
    bool listed = g.min_th <= g.ini_th && nnz <= FC_NZ && bncells <= ORB_BAND_CELLS;
    if (listed) {
        // the local maxima go to one bucket of `kept` per cell, so that the row-major rank of a keypoint inside its
        // cell only scans the maxima of that cell (a fifth of the band's on the EuRoC-shaped frames)
        // ((FC_KEPT / bncells) - 1) | 1, odd: the buckets start in different LDS banks.  By selects on the scalar cell count (1..4 here): the
        // division, and the reciprocal of the pitch that used to follow it, stood between the list's first read and the neighbours' reads
        static_assert(ORB_BAND_CELLS == 4, "cap_c by cell count");
#define FC_CAP(n) (((FC_KEPT / (n)) - 1) | 1)
        const int cap_c = bncells <= 1 ? FC_CAP(1) : bncells == 2 ? FC_CAP(2) : bncells == 3 ? FC_CAP(3) : FC_CAP(4);
#undef FC_CAP
        for (int e = tid; e < nnz; e += FC_TPB) {
            const int pos = e == tid ? nz0 : nz[e];
            // pos / P == (pos / 4) / PW by the band record's multiply-shift: pos / 4 < bh * PW, the staging loop's own range
            const int row = (int)(((unsigned)(pos >> 2) * pw_inv) >> 20), col = pos - row * P;
            // the score, its eight neighbours and the column's cell are read together (one LDS round trip; the tile has a 3-pixel
            // margin around every detection pixel) and the neighbours outside the cell's rectangle masked afterwards: no
            // short-circuit chain of dependent LDS reads
            const uint8_t* p = S + pos;
            const int cc = colcell[col];
            const int sc = p[0];
            const int nl = p[-1], nr = p[1], nul = p[-P - 1], nu = p[-P], nur = p[-P + 1], ndl = p[P - 1], nd = p[P], ndr = p[P + 1];
            __builtin_amdgcn_sched_barrier(0);
            if (cc == 255) continue;
            const int ci = cc & 3, yy = row - 3;
            const bool l = (cc & 4) != 0, r = (cc & 8) != 0, u = yy > 0, d = yy + 1 < rh;
#define NB(c, v) ((c) ? (v) : 0)
            const bool keep = (sc > NB(l, nl)) & (sc > NB(r, nr)) &
                              (sc > NB(u && l, nul)) & (sc > NB(u, nu)) & (sc > NB(u && r, nur)) &
                              (sc > NB(d && l, ndl)) & (sc > NB(d, nd)) & (sc > NB(d && r, ndr));
#undef NB
            if (keep) {
                const int q = atomicAdd(cell_k + ci, 1);
                // yy << 16 | tile column << 8 | score: col < 256 (the colcell table holds every column of the tile), yy <= 58 (the
                // largest band the reciprocals allow has 65 rows), score <= 255.  The row-major order inside a cell is that of
                // (yy, xx): col = clo + xx with one clo per cell.
                if (q < cap_c) kept[ci * cap_c + q] = ((unsigned)yy << 16) | ((unsigned)col << 8) | (unsigned)sc;
                if (sc >= g.ini_th) atomicAdd(cell_hi + ci, 1);
            }
        }
        __syncthreads();
        FC_STAMP(3);
        // (cell_k of the cells the band does not have is 0)
        const int4 ck = *reinterpret_cast<const int4*>(cell_k);
        const int e1 = ck.x, e2 = e1 + ck.y, e3 = e2 + ck.z, nk = e3 + ck.w;
        listed = max(max(ck.x, ck.y), max(ck.z, ck.w)) <= cap_c;
        if (listed) {
            // a cell's count = its local maxima at the chosen threshold.  Every bucket entry is >= minThFAST (stored scores are
            // >= t_lo == minThFAST here) and cell_hi counts those >= iniThFAST, so the count is cell_hi where the cell has any such
            // maximum (threshold iniThFAST) and the whole bucket otherwise (threshold minThFAST); no bucket overflowed on this path.
            // (Until round 3 an atomic per keypoint and a barrier before the store; then one thread per cell scanning its bucket.)
            if (tid >= FC_TPB - FC_CELLS && FC_TPB - 1 - tid < bncells) {
                const int ci = FC_TPB - 1 - tid;
                const int hi = cell_hi[ci];
                g.cell_count[(long long)f * g.ncells + bcfirst + ci] = hi > 0 ? hi : cell_k[ci];
            }
            for (int e = tid; e < nk; e += FC_TPB) {
                const int ci = (e >= e1 ? 1 : 0) + (e >= e2 ? 1 : 0) + (e >= e3 ? 1 : 0);
                const int k0 = e - (ci == 0 ? 0 : ci == 1 ? e1 : ci == 2 ? e2 : e3);
                const unsigned* bucket = kept + ci * cap_c;
                const int nb = ci == 0 ? ck.x : ci == 1 ? ck.y : ci == 2 ? ck.z : ck.w;
                const unsigned me = bucket[k0];
                const unsigned th = (unsigned)(cell_hi[ci] > 0 ? g.ini_th : g.min_th);      // :978-984: ini first, else min
                if ((me & 255u) < th) continue;
                int rank = 0;                                                             // row-major order inside the cell
                for (int k = 0; k < nb; k++) {
                    const unsigned o = bucket[k];
                    rank += ((o & 255u) >= th && (o >> 8) < (me >> 8)) ? 1 : 0;
                }
                const int2 sl = l_slot[ci];                                               // (first slot, slots: one read, one trip)
                if (rank < sl.y)
                    g.slots[(long long)f * g.slots_per_frame + sl.x + rank] =
                        ((me & 255u) << 24) | ((unsigned)(by0 + 3 - ORB_BORDER + (int)((me >> 16) & 63u)) << 12) |
                        (unsigned)(bxa - ORB_BORDER + (int)((me >> 8) & 255u));
            }
            FC_STAMP(4);
            return;
        }
    }
    // ---- per cell: threshold choice, strict 3x3 NMS inside the cell's detection rectangle, ordered compaction
    for (int ci = wv; ci < B.ncells; ci += FC_TPB / 64) {
        const OrbCell c = g.cells[B.cell_first + ci];
        const int rw = c.cw - 6, rh = c.ch - 6;
        int* count_out = g.cell_count + (long long)f * g.ncells + B.cell_first + ci;
        if (rw <= 0 || rh <= 0) { if (lane == 0) *count_out = 0; continue; }
        const uint8_t* S0 = S + 3 * P + (c.x0 + 3 - B.xa);                    // score of the rectangle's first pixel
        unsigned* out = g.slots + (long long)f * g.slots_per_frame + c.slot_first;
        const int relx = c.x0 + 3 - ORB_BORDER, rely = c.y0 + 3 - ORB_BORDER;
        const int rpi = rw <= 32 ? 2 : 1;
        const int xx = rpi == 2 ? (lane & 31) : lane, yoff = rpi == 2 ? (lane >> 5) : 0;
        int n = 0;
        for (int attempt = 0; attempt < 2 && n == 0; attempt++) {
            const int th = attempt == 0 ? g.ini_th : g.min_th;
            for (int y0 = 0; y0 < rh; y0 += rpi) {
                const int yy = y0 + yoff;
                const bool in = yy < rh && xx < rw;
                const uint8_t* p = S0 + min(yy, rh - 1) * P + min(xx, rw - 1);
                const int s = in ? p[0] : 0;
                if (__ballot(s >= th && s > 0) == 0ull) continue;              // most rows hold no corner
                bool keep = false;
                if (s >= th && s > 0) {
                    // neighbours outside the cell's rectangle, and scores below the threshold, count as 0
                    const bool l = xx > 0, r = xx + 1 < rw, u = yy > 0, d = yy + 1 < rh;
#define NB(c, o) ((c) && (int)p[o] >= th ? (int)p[o] : 0)
                    keep = s > NB(l, -1) && s > NB(r, 1) &&
                           s > NB(u && l, -P - 1) && s > NB(u, -P) && s > NB(u && r, -P + 1) &&
                           s > NB(d && l, P - 1) && s > NB(d, P) && s > NB(d && r, P + 1);
#undef NB
                }
                const unsigned long long m = __ballot(keep);
                if (keep) {
                    const int pos = n + __popcll(m & lanemask_lt());
                    if (pos < c.slot_cap)
                        out[pos] = ((unsigned)s << 24) | ((unsigned)(rely + yy) << 12) | (unsigned)(relx + xx);
                }
                n += __popcll(m);
            }
        }
        if (lane == 0) *count_out = n;
    }
}

void orb_launch_fast_cells(hipStream_t s, const OrbGeom& g_dev, const OrbCell* cells, const OrbBand* bands, int nbands, int nframes,
                           size_t lds_bytes, unsigned* slots, int* cell_count, int* clear_status)
{
    // default 0 for this kernel: co-locating neighbouring bands on one XCD cuts its fabric reads 2.2x (285 -> 128 MiB per launch, = the
    // algorithmic bytes) but the kernel, which is not bandwidth-bound, runs 3-5 % slower with every co-locating order tried
    // (profiles/r02_xcd_order.txt); k_orient_desc gains from it and uses it
    static const int xcd_on = getenv("CCM_ORB_XCD") ? atoi(getenv("CCM_ORB_XCD")) : 0;
    const FcLate late = { g_dev.ini_th, g_dev.min_th, g_dev.ncells, g_dev.slots_per_frame, cells, slots, cell_count, clear_status };
    hipLaunchKernelGGL(k_fast_cells, dim3(nbands, nframes), dim3(FC_TPB), lds_bytes, s, bands, xcd_on, (unsigned)nbands, (unsigned)nframes, g_dev.frame0,
                       g_dev.lv[0].img, g_dev.lv[0].plane, g_dev.lv[0].pitch, late);
}
size_t orb_fast_cells_lds(int pitch, int bh) { return fc_lds_bytes(pitch, bh); }
