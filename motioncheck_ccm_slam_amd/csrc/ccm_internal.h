// ccm_internal.h -- shared between the host-side translation units of libccm_hot.so.
#pragma once
#include <hip/hip_runtime.h>
#include <roctracer/roctx.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <utility>
#include <vector>
#include "../../include/ccm_hot.h"

struct OrbState;
struct MatchState;
struct BaState;
struct CommState;
struct PoseState;
struct Sim3State;
struct Sim3RansacState;
struct InitState;
struct PnpState;
struct MapState;
struct EssState;
struct FrameState;

struct ProfLabel { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; size_t used = 0; };

struct ccm_ctx {
    bool prof_on = false;
    ProfLabel prof[CCM_PROF_COUNT];
    int device = 0;
    hipStream_t stream = nullptr;
    // Two auxiliary streams per context, created on first use and SHARED by its subsystems (ccm_aux_stream below): the runtime maps
    // streams onto a handful of hardware queues (4 by default), and streams that share a queue run one after the other -- when the
    // extractor's copy streams and the bundle adjustment's side stream were separate objects, the fifth stream of the process put the
    // coarse inversion into the PCG's queue and the solve took 30 instead of 18 ms (round 3).
    //   aux[0]  lowest priority: the extractor's uploads, the bundle adjustment's coarse inversion
    //   aux[1]  default priority: the extractor's downloads
    hipStream_t aux[2] = { nullptr, nullptr };
    std::string err;
    OrbState* orb = nullptr;
    MatchState* match = nullptr;
    BaState* ba = nullptr;
    CommState* comm = nullptr;
    PoseState* pose = nullptr;
    Sim3State* sim3 = nullptr;
    Sim3RansacState* sim3_ransac = nullptr;   // batched Sim3Solver: staging and device buffers (sim3_ransac_host.cpp)
    InitState* init = nullptr;                // monocular Initializer: staging and device buffers (init_host.cpp)
    PnpState* pnp = nullptr;                  // batched PnPsolver: staging and device buffers (pnp_host.cpp)
    MapState* map = nullptr;                  // CreateNewMapPoints: staging and device buffers (map_host.cpp)
    EssState* ess = nullptr;
    FrameState* frame = nullptr;   // frame handles: pool, staging, live frames (frame_internal.h)
};

// grow-only device buffer; it owns its memory (freed with it), so it can be moved but not copied
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { release(); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return -1; }
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

int ccm_fail(ccm_ctx* c, int code, const char* fmt, ...);
hipStream_t ccm_aux_stream(ccm_ctx* c, int which);      // nullptr if it cannot be created

#define CCM_HIP(c, expr)                                                                   \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess)                                                             \
            return ccm_fail((c), CCM_E_DEVICE, "%s:%d %s -> %s", __FILE__, __LINE__, #expr, \
                            hipGetErrorString(e__));                                       \
    } while (0)

#define CCM_RESERVE(c, buf, bytes)                                                        \
    do {                                                                                  \
        if ((buf).reserve(bytes))                                                         \
            return ccm_fail((c), CCM_E_NOMEM, "%s:%d device alloc of %zu bytes failed",   \
                            __FILE__, __LINE__, (size_t)(bytes));                         \
    } while (0)

// b holds at least max(bytes, 16) bytes, and the bytes from src are queued for upload on st.
inline int ccm_upload(ccm_ctx* c, DevBuf& b, const void* src, size_t bytes, hipStream_t st)
{
    CCM_RESERVE(c, b, std::max<size_t>(bytes, 16));
    if (bytes) CCM_HIP(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
    return CCM_OK;
}

// Runs body() for an entry point of the C ABI.  No C++ exception may cross the C ABI (std::terminate would take the host process --
// a SLAM server -- down): a failed host allocation (vectors sized by the caller's counts, states created on first use) and anything
// else thrown comes back as a status code.
template <class F> int ccm_guard(ccm_ctx* c, const char* name, F&& body) noexcept
{
    try { return body(); }
    catch (const std::bad_alloc&) { return c ? ccm_fail(c, CCM_E_NOMEM, "%s: host allocation failed", name) : CCM_E_NOMEM; }
    catch (const std::exception& e) { return c ? ccm_fail(c, CCM_E_DEVICE, "%s: %s", name, e.what()) : CCM_E_DEVICE; }
    catch (...) { return c ? ccm_fail(c, CCM_E_DEVICE, "%s: unknown exception", name) : CCM_E_DEVICE; }
}

// Brackets the launches issued while it is alive with two events when profiling is on.  Both events go to c->stream, and what
// bench.py --full sums from them into per-kernel and roofline figures are the times of kernels running ALONE: a caller that spreads
// its launches over a second stream (the extractor's two lanes, orb_extract_lanes in orb_host.cpp) keeps to c->stream while prof_on.
struct ProfScope {
    ccm_ctx* c; int label; hipEvent_t stop = nullptr;
    ProfScope(ccm_ctx* ctx, int lab) : c(ctx), label(lab)
    {
        if (!c->prof_on) return;
        ProfLabel& L = c->prof[label];
        if (L.used == L.ev.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            L.ev.emplace_back(a, b);
        }
        (void)hipEventRecord(L.ev[L.used].first, c->stream);
        stop = L.ev[L.used].second;
        L.used++;
    }
    ~ProfScope() { if (stop) (void)hipEventRecord(stop, c->stream); }
};

// Named range in rocprofv3 --marker-trace / roctracer timelines (the reference's only instrumentation is
// g2o's G2OBatchStatistics, block_solver.hpp:441-453, mirrored by the timers of ccm_ba_result; these ranges show where a
// call's host time goes next to the kernels).  A push/pop pair costs ~50 ns when no tool is attached.
struct RoctxRange {
    bool open = true;
    explicit RoctxRange(const char* name) { roctxRangePushA(name); }
    void end() { if (open) { roctxRangePop(); open = false; } }       // close before the scope ends (early returns still balance)
    ~RoctxRange() { end(); }
    RoctxRange(const RoctxRange&) = delete; RoctxRange& operator=(const RoctxRange&) = delete;
};

void orb_state_free(OrbState*);
void match_state_free(MatchState*);
void ba_state_free(BaState*);
void comm_state_free(ccm_ctx*);
void pose_state_free(PoseState*);
void sim3_state_free(Sim3State*);
void sim3_ransac_state_free(Sim3RansacState*);
void init_state_free(InitState*);
void pnp_state_free(PnpState*);
void map_state_free(MapState*);
void ess_state_free(EssState*);
void frame_state_free(ccm_ctx*);                       // also orphans the frames still alive
