// frame_host.cpp -- C ABI of the frame handles (include/ccm_hot.h "frame handles"): one Frame's features, descriptors, grid and
// map-point ids in device memory, reused by the per-frame matchers and the pose optimisation of Tracking
// (TrackWithMotionModel src/Tracking.cpp:571-597, TrackLocalMap :905-920).
//
// Per call, every input goes into one page-locked staging area of the context laid out like its device twin `io`:
//   [ results | inputs ]   one host-to-device copy of the inputs, the kernels, one device-to-host copy of the results, one
// stream synchronisation.  The results come first so that in/out data (the occupancy flags, the pose) sits at the seam and
// travels both ways without a second copy.
#include "frame_internal.h"
#include "bow_directory.h"
#include <algorithm>
#include <climits>
#include <cstdarg>
#include <new>

struct FrameLayout { size_t kx, ky, oct, angle, desc, upload_end, mp_id, items, first, bytes; };
static FrameLayout frame_layout(int n, int cells)
{
    const size_t m = (size_t)std::max(n, 1);
    FrameLayout L; size_t off = 0;
    L.kx = seg(off, m * 4); L.ky = seg(off, m * 4); L.oct = seg(off, m * 4); L.angle = seg(off, m * 4); L.desc = seg(off, m * 32);
    L.upload_end = off;
    L.mp_id = seg(off, m * 4); L.items = seg(off, m * 4); L.first = seg(off, ((size_t)cells + 1) * 4);
    L.bytes = off;
    return L;
}

FrameState* frame_state(ccm_ctx* c)
{
    if (!c->frame) c->frame = new FrameState();
    return c->frame;
}

void frame_state_free(ccm_ctx* c)
{
    FrameState* S = c->frame;
    if (!S) return;
    mpt_tables_orphan(S);
    for (ccm_frame* f : S->live) {               // frames the caller did not destroy: memory goes, the handle stays (ccm_frame_destroy)
        delete f->mem;
        delete f->kf_mem;
        *f = ccm_frame();
    }
    for (FrameMem* m : S->pool) delete m;
    for (FrameMem* m : S->kf_pool) delete m;
    if (S->host) (void)hipHostFree(S->host);
    if (S->host_free) (void)hipEventDestroy(S->host_free);
    delete S;
    c->frame = nullptr;
}

// The page-locked staging area with at least `bytes`, free to write (the last upload from it has completed), and io as large.
int frame_staging(ccm_ctx* c, size_t bytes, uint8_t** host)
{
    FrameState& S = *frame_state(c);
    if (!S.host_free) CCM_HIP(c, hipEventCreateWithFlags(&S.host_free, hipEventDisableTiming));
    if (S.pending) { CCM_HIP(c, hipEventSynchronize(S.host_free)); S.pending = false; }
    if (bytes > S.host_cap) {
        if (S.host) (void)hipHostFree(S.host);
        S.host = nullptr; S.host_cap = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        if (hipHostMalloc((void**)&S.host, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); S.host = nullptr;
            return ccm_fail(c, CCM_E_NOMEM, "page-locked staging of %zu bytes failed", want);
        }
        S.host_cap = want;
    }
    CCM_RESERVE(c, S.io, bytes);
    *host = S.host;
    return CCM_OK;
}

// host[a, b) -> dst (default: io at the same offsets), asynchronous; the staging area stays busy until the copy has run
int frame_upload(ccm_ctx* c, size_t a, size_t b, void* dst)
{
    FrameState& S = *c->frame;
    if (b <= a) return CCM_OK;
    CCM_HIP(c, hipMemcpyAsync(dst ? dst : S.io.as<uint8_t>() + a, S.host + a, b - a, hipMemcpyHostToDevice, c->stream));
    CCM_HIP(c, hipEventRecord(S.host_free, c->stream));
    S.pending = true;
    return CCM_OK;
}

// io[0, b) -> host[0, b), then wait for the stream
int frame_download(ccm_ctx* c, size_t b)
{
    FrameState& S = *c->frame;
    CCM_HIP(c, hipMemcpyAsync(S.host, S.io.p, b, hipMemcpyDeviceToHost, c->stream));
    CCM_HIP(c, hipStreamSynchronize(c->stream));
    S.pending = false;
    return CCM_OK;
}

int frame_fetch(ccm_ctx* c, void* dst, const void* src_dev, size_t bytes)   // rare paths (fallbacks, test taps)
{
    if (!bytes) return CCM_OK;
    CCM_HIP(c, hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    CCM_HIP(c, hipStreamSynchronize(c->stream));
    return CCM_OK;
}

// Best fit among the free blocks, else the largest one (the caller grows it), else a new block.
static FrameMem* pool_take(std::vector<FrameMem*>& pool, size_t bytes)
{
    int pick = -1;
    for (int i = 0; i < (int)pool.size(); i++)
        if (pool[i]->buf.cap >= bytes && (pick < 0 || pool[i]->buf.cap < pool[pick]->buf.cap)) pick = i;
    if (pick < 0)
        for (int i = 0; i < (int)pool.size(); i++) if (pick < 0 || pool[i]->buf.cap > pool[pick]->buf.cap) pick = i;
    if (pick < 0) return new FrameMem();
    FrameMem* m = pool[pick];
    pool.erase(pool.begin() + pick);
    return m;
}

static int frame_alloc(ccm_ctx* c, int n, int cols, int rows, ccm_frame** out)
{
    FrameState& S = *frame_state(c);
    const FrameLayout L = frame_layout(n, cols * rows);
    FrameMem* m = pool_take(S.pool, L.bytes);
    if (m->buf.reserve(L.bytes)) {
        S.pool.push_back(m);
        return ccm_fail(c, CCM_E_NOMEM, "frame: device alloc of %zu bytes failed", L.bytes);
    }
    ccm_frame* f = new ccm_frame();
    uint8_t* base = m->buf.as<uint8_t>();
    f->ctx = c; f->mem = m; f->n = n; f->cols = cols; f->rows = rows;
    f->kx = (float*)(base + L.kx); f->ky = (float*)(base + L.ky); f->oct = (int*)(base + L.oct); f->angle = (float*)(base + L.angle);
    f->desc = base + L.desc; f->mp_id = (int*)(base + L.mp_id); f->cell_items = (int*)(base + L.items); f->cell_first = (int*)(base + L.first);
    S.live.push_back(f);
    *out = f;
    return CCM_OK;
}

static void frame_release(ccm_frame* f)
{
    if (f->ctx && f->ctx->frame) {
        FrameState& S = *f->ctx->frame;
        S.live.erase(std::remove(S.live.begin(), S.live.end(), f), S.live.end());
        if (f->mem) S.pool.push_back(f->mem);    // stream order keeps queued work on it ahead of the next user
        if (f->kf_mem) S.kf_pool.push_back(f->kf_mem);
    }
    delete f;
}

static int frame_build(ccm_ctx* c, ccm_frame* f, const ccm_keypoint* kps, const uint8_t* src_desc, int keep_xy)
{
    FrameBuildArgs A{ f->n, f->cols, f->rows, f->min_x, f->min_y, f->inv_w, f->inv_h, kps, src_desc, keep_xy,
                      f->kx, f->ky, f->oct, f->angle, f->desc, f->cell_first, f->cell_items, f->mp_id };
    if (frame_launch_build(c->stream, A)) return ccm_fail(c, CCM_E_DEVICE, "k_frame_build: LDS request refused");
    CCM_HIP(c, hipGetLastError());
    return CCM_OK;
}

static bool grid_ok(int cols, int rows) { return cols >= 1 && rows >= 1 && (long long)cols * rows <= 16384; }

// The windowed matchers through a handle.  mode 0: SearchByProjection(Frame, map points); mode 2: SearchByProjection(Frame,
// Frame | KeyFrame).  Queries come with their radius / level window (qr != nullptr) or, for a `last` handle, get them on the device.
struct WinCall {
    int mode, nq;
    const float* qx; const float* qy; const float* qr; const int32_t* minl; const int32_t* maxl;
    const uint8_t* qdesc; const uint8_t* active; const uint8_t* qflag; const int32_t* qid;
    const ccm_frame* last; const float* scale; float th;      // device-side query set-up (qr == nullptr)
    const float* q_angle;                                     // mode 2, check_ori, no `last`: the last side's angles (host)
    float nnratio; int orb_dist, check_ori;
};

static int frame_window(ccm_ctx* c, ccm_frame* f, const WinCall& w, uint8_t* occupied, int32_t* match)
{
    FrameState& S = *frame_state(c);
    hipStream_t st = c->stream;
    const int n = f->n, nq = w.nq;
    const bool dev_prep = w.qr == nullptr;
    const bool need_qang = w.mode == 2 && w.check_ori && !w.last;
    size_t off = 0;
    const size_t o_status = seg(off, 16), o_out = seg(off, (size_t)n * 4), o_flag = seg(off, (size_t)n);
    const size_t res_end = o_flag + n;
    const size_t o_qx = seg(off, (size_t)nq * 4), o_qy = seg(off, (size_t)nq * 4), o_qr = seg(off, (size_t)nq * 4);
    const size_t o_minl = seg(off, (size_t)nq * 4), o_maxl = seg(off, (size_t)nq * 4), o_qdesc = seg(off, (size_t)nq * 32);
    const size_t o_act = seg(off, (size_t)nq), o_qflag = seg(off, (size_t)nq);
    const size_t o_qid = seg(off, w.qid ? (size_t)nq * 4 : 0), o_qang = seg(off, need_qang ? (size_t)nq * 4 : 0);
    const size_t o_scale = seg(off, dev_prep ? (size_t)w.last->n_levels * 4 : 0);
    const size_t end = off;
    uint8_t* h = nullptr;
    int rc = frame_staging(c, end, &h);
    if (rc) return rc;
    std::memset(h + o_out, 0xFF, (size_t)n * 4);
    std::memcpy(h + o_flag, occupied, n);
    std::memcpy(h + o_qx, w.qx, (size_t)nq * 4); std::memcpy(h + o_qy, w.qy, (size_t)nq * 4);
    if (!dev_prep) {
        std::memcpy(h + o_qr, w.qr, (size_t)nq * 4); std::memcpy(h + o_minl, w.minl, (size_t)nq * 4); std::memcpy(h + o_maxl, w.maxl, (size_t)nq * 4);
    } else {
        std::memcpy(h + o_scale, w.scale, (size_t)w.last->n_levels * 4);
    }
    std::memcpy(h + o_qdesc, w.qdesc, (size_t)nq * 32);
    std::memcpy(h + o_act, w.active, nq); std::memcpy(h + o_qflag, w.qflag, nq);
    if (w.qid) std::memcpy(h + o_qid, w.qid, (size_t)nq * 4);
    if (need_qang) std::memcpy(h + o_qang, w.q_angle, (size_t)nq * 4);
    if ((rc = frame_upload(c, o_out, end))) return rc;

    uint8_t* io = S.io.as<uint8_t>();
    float* d_qr = (float*)(io + o_qr); int* d_minl = (int*)(io + o_minl); int* d_maxl = (int*)(io + o_maxl);
    const uint8_t* d_act = io + o_act;
    const int* d_qid = w.qid ? (const int*)(io + o_qid) : nullptr;
    if (dev_prep) {
        frame_launch_prep_last(st, nq, d_act, w.last->oct, (const float*)(io + o_scale), w.th, d_qr, d_minl, d_maxl);
        CCM_HIP(c, hipGetLastError());
    }
    WinDevCall D{ w.mode, nq, (const float*)(io + o_qx), (const float*)(io + o_qy), d_qr, d_minl, d_maxl, io + o_qdesc, d_act, io + o_qflag,
                  d_qid ? d_qid : (w.last ? w.last->mp_id : nullptr),
                  need_qang ? (const float*)(io + o_qang) : (w.last ? w.last->angle : nullptr),
                  o_status, o_out, o_flag, res_end, w.nnratio, w.orb_dist, w.check_ori, w.active, w.qflag, w.q_angle, w.last, nullptr, false };
    return frame_window_dev(c, f, D, occupied, match);
}

int frame_window_dev(ccm_ctx* c, ccm_frame* f, WinDevCall& w, uint8_t* occupied, int32_t* match)
{
    FrameState& S = *frame_state(c);
    hipStream_t st = c->stream;
    const int n = f->n, nq = w.nq;
    const size_t o_status = w.o_status, o_out = w.o_out, o_flag = w.o_flag, res_end = w.res_end;
    uint8_t* io = S.io.as<uint8_t>();
    int* d_status = (int*)(io + o_status); int* d_out = (int*)(io + o_out); uint8_t* d_flag = io + o_flag;
    const float* d_qx = w.qx; const float* d_qy = w.qy; const float* d_qr = w.qr; const int* d_minl = w.minl; const int* d_maxl = w.maxl;
    const uint8_t* d_qdesc = w.qdesc; const uint8_t* d_act = w.act; const uint8_t* d_qflag = w.qflag;
    const float* d_qang = w.qang; const int* id_src = w.id_src;
    int rc;
    w.host_accept = false;
    const WinGrid G = frame_win_grid(f);
    auto lists = [&](int cap) -> int {
        CCM_RESERVE(c, S.ci, (size_t)nq * cap * 4); CCM_RESERVE(c, S.cd, (size_t)nq * cap * 4); CCM_RESERVE(c, S.cn, (size_t)nq * 4);
        match_launch_window(st, G, nq, d_qx, d_qy, d_qr, d_minl, d_maxl, d_qdesc, cap, S.ci.as<int>(), S.cd.as<int>(), S.cn.as<int>());
        CCM_HIP(c, hipGetLastError());
        return CCM_OK;
    };

    if (!window_host_accept_forced() && match_window_greedy_lds(n, nq) <= kGreedyLdsMax) {
        int cap = 64;
        CCM_RESERVE(c, S.ev, std::max<size_t>((size_t)nq * 4, 16));
        for (int attempt = 0; attempt < 3; attempt++) {
            if ((rc = lists(cap))) return rc;
            GreedyArgs A{ nq, n, cap, S.ci.as<int>(), S.cd.as<int>(), S.cn.as<int>(), d_act, nullptr, f->oct, d_qflag, d_flag, w.nnratio,
                          d_out, d_status, w.orb_dist, w.check_ori, d_qang, f->angle, S.ev.as<int>(), nullptr };
            if (match_launch_window_greedy(st, w.mode, A)) return ccm_fail(c, CCM_E_DEVICE, "k_window_greedy: LDS request refused");
            CCM_HIP(c, hipGetLastError());
            frame_launch_scatter_ids(st, n, d_out, id_src, d_status, f->mp_id);
            if (w.ids_copy) frame_launch_scatter_ids(st, n, d_out, id_src, d_status, w.ids_copy);
            CCM_HIP(c, hipGetLastError());
            if ((rc = frame_download(c, res_end))) return rc;
            int status[2];
            std::memcpy(status, S.host + o_status, 8);
            if (status[0] < 0) { cap = status[1]; continue; }                  // rare: a denser window than expected
            std::memcpy(match, S.host + o_out, (size_t)n * 4);
            std::memcpy(occupied, S.host + o_flag, n);
            return status[0];
        }
        return ccm_fail(c, CCM_E_CAPACITY, "window candidate lists keep overflowing");
    }

    // host acceptance (CCM_WINDOW_HOST_ACCEPT=1, or a frame too large for the single workgroup's LDS): lists to the host, the loops
    // of match_window_host.cpp on the frame's octaves / angles fetched from the device, the new ids scattered on the device
    w.host_accept = true;
    std::vector<uint8_t> act_h, qflag_h;
    const uint8_t* h_act = w.h_act; const uint8_t* h_qflag = w.h_qflag;
    if (!h_act) {                                                              // queries made on the device: their flags come back too
        act_h.resize(nq); qflag_h.resize(nq);
        if ((rc = frame_fetch(c, act_h.data(), d_act, nq)) || (rc = frame_fetch(c, qflag_h.data(), d_qflag, nq)) ||
            (rc = frame_fetch(c, occupied, d_flag, n))) return rc;
        h_act = act_h.data(); h_qflag = qflag_h.data();
        for (int i = 0; i < n; i++) match[i] = -1;
    }
    int cap = 64;
    std::vector<int32_t> ci, cd, cn(nq);
    for (;;) {
        if ((rc = lists(cap))) return rc;
        ci.resize((size_t)nq * cap); cd.resize((size_t)nq * cap);
        if ((rc = frame_fetch(c, cn.data(), S.cn.p, (size_t)nq * 4))) return rc;
        int mx = 0;
        for (int v : cn) mx = std::max(mx, v);
        if (mx > cap) { cap = mx; continue; }
        if ((rc = frame_fetch(c, ci.data(), S.ci.p, ci.size() * 4)) || (rc = frame_fetch(c, cd.data(), S.cd.p, cd.size() * 4))) return rc;
        break;
    }
    int nmatches;
    if (w.mode == 0) {
        std::vector<int32_t> oct(n);
        if ((rc = frame_fetch(c, oct.data(), f->oct, (size_t)n * 4))) return rc;
        nmatches = window_accept_projection_host(nq, h_act, ci.data(), cd.data(), cn.data(), cap, oct.data(), h_qflag, occupied, w.nnratio, match);
    } else {
        std::vector<float> cur_angle, last_angle;
        if (w.check_ori) {
            cur_angle.resize(n);
            if ((rc = frame_fetch(c, cur_angle.data(), f->angle, (size_t)n * 4))) return rc;
            if (w.last) { last_angle.resize(nq); if ((rc = frame_fetch(c, last_angle.data(), w.last->angle, (size_t)nq * 4))) return rc; }
        }
        nmatches = window_accept_frame_host(nq, h_act, ci.data(), cd.data(), cn.data(), cap, h_qflag, occupied, w.orb_dist, w.check_ori,
                                            w.last ? last_angle.data() : w.h_qang, cur_angle.data(), match);
    }
    std::memcpy(S.host + o_out, match, (size_t)n * 4);                       // the stream is idle: the staging area is free
    if ((rc = frame_upload(c, o_out, o_out + (size_t)n * 4))) return rc;
    frame_launch_scatter_ids(st, n, d_out, id_src, nullptr, f->mp_id);
    CCM_HIP(c, hipGetLastError());
    return nmatches;
}

// ---- the keyframe part of a handle
struct KfLayout { size_t node, order, nodes, first, bow_end, feat, desc, sf, sig2, cam, bytes; };
static KfLayout kf_layout(int n)
{
    const size_t m = (size_t)std::max(n, 1);
    KfLayout L; size_t off = 0;
    L.node = seg(off, m * 4); L.order = seg(off, m * 4); L.nodes = seg(off, m * 4); L.first = seg(off, (m + 1) * 4);
    L.bow_end = off;
    L.feat = seg(off, m * sizeof(MapFeat)); L.desc = seg(off, m * 32);
    L.sf = seg(off, ccm_frame::kMaxLevels * 4); L.sig2 = seg(off, ccm_frame::kMaxLevels * 4); L.cam = seg(off, sizeof(MapCam));
    L.bytes = off;
    return L;
}

// The handle's second block, taken from the pool of keyframe parts on the first setter.
static int kf_block(ccm_ctx* c, ccm_frame* f)
{
    if (f->kf_mem) return CCM_OK;
    FrameState& S = *frame_state(c);
    const KfLayout L = kf_layout(f->n);
    FrameMem* m = pool_take(S.kf_pool, L.bytes);
    if (m->buf.reserve(L.bytes)) {
        S.kf_pool.push_back(m);
        return ccm_fail(c, CCM_E_NOMEM, "frame: device alloc of %zu bytes failed", L.bytes);
    }
    uint8_t* base = m->buf.as<uint8_t>();
    f->kf_mem = m;
    f->node = (int*)(base + L.node); f->order = (int*)(base + L.order); f->nodes = (int*)(base + L.nodes); f->first = (int*)(base + L.first);
    f->feat_o = (MapFeat*)(base + L.feat); f->desc_o = base + L.desc; f->sf = (float*)(base + L.sf); f->sig2 = (float*)(base + L.sig2);
    f->d_cam = (MapCam*)(base + L.cam);
    return CCM_OK;
}

// The node-ordered copies, once bow and camera are both there (whichever came last)
static int kf_gather(ccm_ctx* c, ccm_frame* f)
{
    if (!f->has_bow || !f->has_cam || f->n_bow == 0) return CCM_OK;
    frame_launch_kf_gather(c->stream, KfGatherArgs{ f->n_bow, f->order, f->kx, f->ky, f->oct, f->desc, f->sf, f->sig2, f->feat_o, f->desc_o });
    CCM_HIP(c, hipGetLastError());
    return CCM_OK;
}

// The node directory built on the host from node[n] (bow_directory.h) and sent to the handle's keyframe block in one copy:
// ccm_frame_set_bow, and ccm_frame_compute_bow for a frame above kBowDirMax.  On an argument error the handle keeps its bow.
static int bow_install(ccm_ctx* c, ccm_frame* f, const int32_t* node, const char* fn)
{
    const int n = f->n;
    if (n > (1 << 20) - 1) return ccm_fail(c, CCM_E_ARG, "%s: n = %d above %d", fn, n, (1 << 20) - 1);
    for (int i = 0; i < n; i++)
        if (node[i] >= (1 << 24)) return ccm_fail(c, CCM_E_ARG, "%s: node[%d] = %d, not below %d", fn, i, node[i], 1 << 24);
    BowDirectory D;
    bow_directory_build(node, n, D);
    CCM_HIP(c, hipSetDevice(c->device));
    int rc = kf_block(c, f);
    if (rc) return rc;
    const KfLayout L = kf_layout(n);
    uint8_t* h = nullptr;
    if ((rc = frame_staging(c, L.bow_end, &h))) return rc;
    std::memcpy(h + L.node, node, (size_t)n * 4);
    std::memcpy(h + L.order, D.order.data(), D.order.size() * 4);
    std::memcpy(h + L.nodes, D.nodes.data(), D.nodes.size() * 4);
    std::memcpy(h + L.first, D.first.data(), D.first.size() * 4);
    // the copy is queued over the live directory before the event record that can still fail: then the handle has no bow at all
    if ((rc = frame_upload(c, 0, L.bow_end, f->kf_mem->buf.p))) { f->has_bow = false; return rc; }
    f->has_bow = true; f->n_bow = (int)D.order.size(); f->n_nodes = (int)D.nodes.size();
    return kf_gather(c, f);
}

const char* frame_keyframe_lacks(const ccm_frame* f) { return !f->has_bow ? "bow" : !f->has_cam ? "camera" : !f->has_pose ? "pose" : nullptr; }

int frame_check(ccm_ctx* c, const ccm_frame* f)
{
    if (!f->ctx) return ccm_fail(c, CCM_E_ARG, "frame handle outlived its context");
    if (f->ctx != c) return ccm_fail(c, CCM_E_ARG, "frame handle belongs to another context");
    return CCM_OK;
}

int frame_named_check(ccm_ctx* c, const ccm_frame* f, const char* fn, const char* who, ...)
{
    char name[48];
    va_list ap;
    va_start(ap, who);
    vsnprintf(name, sizeof name, who, ap);
    va_end(ap);
    if (!f) return ccm_fail(c, CCM_E_ARG, "%s: %s is null", fn, name);
    if (!f->ctx) return ccm_fail(c, CCM_E_STATE, "%s: %s outlived its context", fn, name);
    if (f->ctx != c) return ccm_fail(c, CCM_E_ARG, "%s: %s belongs to another context", fn, name);
    return CCM_OK;
}

int frame_pose_queue(ccm_ctx* c, ccm_frame* f, int n_mp, const float* pos, const uint8_t* flags, int n_levels, const PoseIo& o)
{
    FrameState& S = *frame_state(c);
    hipStream_t st = c->stream;
    const int n = f->n;
    CCM_RESERVE(c, S.pts, (size_t)n * 24); CCM_RESERVE(c, S.obs, (size_t)n * 16); CCM_RESERVE(c, S.info, (size_t)n * 8);
    CCM_RESERVE(c, S.err, (size_t)n * 16); CCM_RESERVE(c, S.outl, (size_t)n); CCM_RESERVE(c, S.kof, (size_t)n * 4); CCM_RESERVE(c, S.first, 16);
    uint8_t* io = S.io.as<uint8_t>();
    int* d_ninl = (int*)(io + o.ninl); int* d_status = d_ninl + 1;
    PoseGatherArgs G{ n, f->kx, f->ky, f->oct, f->mp_id, n_mp, (const double*)(io + o.xyz), pos, flags, (const float*)(io + o.is2), n_levels,
                      S.first.as<int>(), S.pts.as<double>(), S.obs.as<double>(), S.info.as<double>(), S.kof.as<int>(), d_status };
    frame_launch_pose_gather(st, G);
    CCM_HIP(c, hipGetLastError());
    PoseDev D{ 1, (double*)(io + o.pose), (const double*)(io + o.intr), S.first.as<int>(), S.pts.as<double>(), S.obs.as<double>(),
               S.info.as<double>(), S.err.as<double>(), S.outl.as<uint8_t>(), d_ninl };
    pose_launch(st, D);
    CCM_HIP(c, hipGetLastError());
    frame_launch_pose_scatter(st, n, S.kof.as<int>(), S.first.as<int>(), S.outl.as<uint8_t>(), io + o.outl);
    CCM_HIP(c, hipGetLastError());
    return CCM_OK;
}

int frame_pose_run(ccm_ctx* c, ccm_frame* f, int n_mp, const double* mp_xyz, const float* pos, const uint8_t* flags,
                   const float* inv_level_sigma2, int n_levels, const double intr[4], double pose7[7], uint8_t* outlier, int32_t* n_inliers,
                   bool* bad_id)
{
    CCM_HIP(c, hipSetDevice(c->device));
    FrameState& S = *frame_state(c);
    const int n = f->n;
    const size_t xyz_bytes = mp_xyz ? (size_t)n_mp * 24 : 0;
    size_t off = 0;
    const size_t o_ninl = seg(off, 16), o_outl = seg(off, (size_t)n), o_pose = seg(off, 56);
    const size_t res_end = o_pose + 56;
    const size_t o_intr = seg(off, 32), o_is2 = seg(off, (size_t)n_levels * 4), o_xyz = seg(off, xyz_bytes);
    const size_t end = off;
    uint8_t* h = nullptr;
    int rc;
    if ((rc = frame_staging(c, end, &h))) return rc;
    std::memcpy(h + o_pose, pose7, 56); std::memcpy(h + o_intr, intr, 32);
    std::memcpy(h + o_is2, inv_level_sigma2, (size_t)n_levels * 4);
    if (xyz_bytes) std::memcpy(h + o_xyz, mp_xyz, xyz_bytes);
    if ((rc = frame_upload(c, o_pose, end))) return rc;
    if ((rc = frame_pose_queue(c, f, n_mp, pos, flags, n_levels, PoseIo{ o_ninl, o_outl, o_pose, o_intr, o_is2, o_xyz }))) return rc;
    if ((rc = frame_download(c, res_end))) return rc;
    int head[2];
    std::memcpy(head, S.host + o_ninl, 8);
    *bad_id = head[1] != 0;
    if (*bad_id) return CCM_OK;
    std::memcpy(pose7, S.host + o_pose, 56);
    std::memcpy(outlier, S.host + o_outl, n);
    *n_inliers = head[0];
    return CCM_OK;
}

extern "C" {

int ccm_frame_create(ccm_ctx* c, const ccm_frame_grid* g, const float* angle, ccm_frame** out)
{
    RoctxRange roctx_("ccm_frame_create");
    if (out) *out = nullptr;
    if (!c || !g || !out) return CCM_E_ARG;
    if (g->n < 0 || !grid_ok(g->grid_cols, g->grid_rows) || (g->n > 0 && (!g->kp_x || !g->kp_y || !g->kp_octave || !g->desc)))
        return ccm_fail(c, CCM_E_ARG, "bad frame arguments (grid of at most 16384 cells)");
    return ccm_guard(c, "ccm_frame_create", [&]() -> int {
        int max_oct = -1;
        for (int i = 0; i < g->n; i++) {
            if (g->kp_octave[i] < 0 || g->kp_octave[i] > 255) return ccm_fail(c, CCM_E_ARG, "octave of feature %d out of [0, 255]", i);
            max_oct = std::max(max_oct, (int)g->kp_octave[i]);
        }
        CCM_HIP(c, hipSetDevice(c->device));
        const int n = g->n;
        const FrameLayout L = frame_layout(n, g->grid_cols * g->grid_rows);
        uint8_t* h = nullptr;
        int rc = frame_staging(c, L.upload_end, &h);
        if (rc) return rc;
        std::memcpy(h + L.kx, g->kp_x, (size_t)n * 4); std::memcpy(h + L.ky, g->kp_y, (size_t)n * 4);
        std::memcpy(h + L.oct, g->kp_octave, (size_t)n * 4);
        if (angle) std::memcpy(h + L.angle, angle, (size_t)n * 4);
        else std::memset(h + L.angle, 0, (size_t)n * 4);
        std::memcpy(h + L.desc, g->desc, (size_t)n * 32);
        ccm_frame* f = nullptr;
        if ((rc = frame_alloc(c, n, g->grid_cols, g->grid_rows, &f))) return rc;
        f->n_levels = max_oct + 1; f->has_angle = angle != nullptr;
        f->min_x = g->min_x; f->min_y = g->min_y; f->inv_w = g->inv_w; f->inv_h = g->inv_h;
        if ((rc = frame_upload(c, 0, L.upload_end, f->mem->buf.p)) || (rc = frame_build(c, f, nullptr, nullptr, 0))) { frame_release(f); return rc; }
        *out = f;
        return CCM_OK;
    });
}

int ccm_frame_from_extract(ccm_ctx* c, int image, int n, const float* kp_x_un, const float* kp_y_un, float min_x, float min_y,
                           float inv_w, float inv_h, int grid_cols, int grid_rows, ccm_frame** out)
{
    RoctxRange roctx_("ccm_frame_from_extract");
    if (out) *out = nullptr;
    if (!c || !out) return CCM_E_ARG;
    if (!grid_ok(grid_cols, grid_rows) || (!kp_x_un) != (!kp_y_un) || n < -1)
        return ccm_fail(c, CCM_E_ARG, "bad frame arguments (grid of at most 16384 cells, both or neither coordinate array)");
    return ccm_guard(c, "ccm_frame_from_extract", [&]() -> int {
        const ccm_keypoint* kps = nullptr; const uint8_t* desc = nullptr; const int32_t* counts = nullptr;
        int n_images = 0, max_per_image = 0, nlevels = 0;
        int rc = orb_last_result(c, &kps, &desc, &counts, &n_images, &max_per_image, &nlevels);
        if (rc) return rc;
        if (image < 0 || image >= n_images) return ccm_fail(c, CCM_E_ARG, "image %d out of range [0, %d)", image, n_images);
        if (n > max_per_image) return ccm_fail(c, CCM_E_ARG, "n %d above the extract's max_per_image %d", n, max_per_image);
        CCM_HIP(c, hipSetDevice(c->device));
        if (n < 0) {
            int32_t cnt = 0;
            if ((rc = frame_fetch(c, &cnt, counts + image, 4))) return rc;
            n = std::min<int>(cnt, max_per_image);
        }
        const FrameLayout L = frame_layout(n, grid_cols * grid_rows);
        if (kp_x_un) {
            uint8_t* h = nullptr;
            if ((rc = frame_staging(c, L.oct, &h))) return rc;
            std::memcpy(h + L.kx, kp_x_un, (size_t)n * 4); std::memcpy(h + L.ky, kp_y_un, (size_t)n * 4);
        }
        ccm_frame* f = nullptr;
        if ((rc = frame_alloc(c, n, grid_cols, grid_rows, &f))) return rc;
        f->n_levels = nlevels; f->has_angle = true;
        f->min_x = min_x; f->min_y = min_y; f->inv_w = inv_w; f->inv_h = inv_h;
        if ((kp_x_un && (rc = frame_upload(c, 0, L.oct, f->mem->buf.p))) ||
            (rc = frame_build(c, f, kps + (size_t)image * max_per_image, desc + (size_t)image * max_per_image * 32, kp_x_un ? 1 : 0))) {
            frame_release(f); return rc;
        }
        *out = f;
        return CCM_OK;
    });
}

void ccm_frame_destroy(ccm_frame* f)
{
    if (!f) return;
    try { frame_release(f); } catch (...) {}
}

int ccm_frame_size(const ccm_frame* f) { return f ? f->n : CCM_E_ARG; }

int ccm_frame_set_map_points(ccm_frame* f, const int32_t* mp_id)
{
    if (!f) return CCM_E_ARG;
    ccm_ctx* c = f->ctx;
    if (!c) return CCM_E_STATE;
    if (f->n == 0) return CCM_OK;
    return ccm_guard(c, "ccm_frame_set_map_points", [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        if (!mp_id) { CCM_HIP(c, hipMemsetAsync(f->mp_id, 0xFF, (size_t)f->n * 4, c->stream)); return CCM_OK; }
        uint8_t* h = nullptr;
        int rc = frame_staging(c, (size_t)f->n * 4, &h);
        if (rc) return rc;
        std::memcpy(h, mp_id, (size_t)f->n * 4);
        return frame_upload(c, 0, (size_t)f->n * 4, f->mp_id);
    });
}

int ccm_frame_get_map_points(ccm_frame* f, int32_t* mp_id)
{
    if (!f || !mp_id) return CCM_E_ARG;
    ccm_ctx* c = f->ctx;
    if (!c) return CCM_E_STATE;
    CCM_HIP(c, hipSetDevice(c->device));
    return frame_fetch(c, mp_id, f->mp_id, (size_t)f->n * 4);
}

int ccm_frame_debug_grid(ccm_frame* f, int32_t* cell_first, int32_t* cell_items)
{
    if (!f || !cell_first || !cell_items) return CCM_E_ARG;
    ccm_ctx* c = f->ctx;
    if (!c) return CCM_E_STATE;
    CCM_HIP(c, hipSetDevice(c->device));
    const int cells = f->cols * f->rows;
    int rc = frame_fetch(c, cell_first, f->cell_first, ((size_t)cells + 1) * 4);
    if (rc) return rc;
    if (cell_first[cells] < 0 || cell_first[cells] > f->n) return ccm_fail(c, CCM_E_DEVICE, "grid of %d items for %d features", cell_first[cells], f->n);
    return frame_fetch(c, cell_items, f->cell_items, (size_t)cell_first[cells] * 4);
}

// KeyFrame::mFeatVec as one node per feature (KeyFrame::ComputeBoW, read by SearchForTriangulation ORBmatcher.cpp:739-805)
int ccm_frame_set_bow(ccm_frame* f, const int32_t* node)
{
    if (!f) return CCM_E_ARG;
    ccm_ctx* c = f->ctx;
    if (!c) return CCM_E_STATE;
    if (!node) { f->has_bow = false; return CCM_OK; }
    return ccm_guard(c, "ccm_frame_set_bow", [&]() -> int { return bow_install(c, f, node, "ccm_frame_set_bow"); });
}

// Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cpp:268-275) on a handle: the vocabulary descent on the handle's own descriptor
// rows, then the node directory built where the nodes already are
int ccm_frame_compute_bow(ccm_ctx* c, ccm_frame* f, ccm_vocabulary* voc, int levelsup, int32_t* word_id, double* weight, int32_t* node)
{
    RoctxRange roctx_("ccm_frame_compute_bow");
    if (!c || !f || !voc) return CCM_E_ARG;
    if (!f->ctx) return ccm_fail(c, CCM_E_STATE, "ccm_frame_compute_bow: frame handle outlived its context");
    int rc = frame_check(c, f);
    if (rc) return rc;
    const VocView V = voc_view(voc);
    if (V.ctx != c) return ccm_fail(c, CCM_E_ARG, "ccm_frame_compute_bow: vocabulary belongs to another context");
    if (V.n_nodes >= (1 << 24)) return ccm_fail(c, CCM_E_ARG, "ccm_frame_compute_bow: vocabulary of %d nodes, not below %d", V.n_nodes, 1 << 24);
    if (f->n > (1 << 20) - 1) return ccm_fail(c, CCM_E_ARG, "ccm_frame_compute_bow: n = %d above %d", f->n, (1 << 20) - 1);
    const bool want = word_id || weight || node;
    if (want && (!word_id || !weight || !node)) return ccm_fail(c, CCM_E_ARG, "ccm_frame_compute_bow: word_id, weight and node come together or not at all");
    return ccm_guard(c, "ccm_frame_compute_bow", [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        FrameState& S = *frame_state(c);
        hipStream_t st = c->stream;
        const int n = f->n;
        const bool empty = V.n_words == 0;                                     // empty(): transform() returns nothing (:1133)
        size_t off = 0;
        const size_t o_cnt = seg(off, 16), o_word = seg(off, (size_t)n * 4), o_leaf = seg(off, (size_t)n * 4), o_node = seg(off, (size_t)n * 4);
        const size_t end = off;
        uint8_t* h = nullptr;
        if ((rc = frame_staging(c, end, &h)) || (rc = kf_block(c, f))) return rc;
        uint8_t* io = S.io.as<uint8_t>();
        int* d_cnt = (int*)(io + o_cnt); int* d_word = (int*)(io + o_word); int* d_leaf = (int*)(io + o_leaf); int* d_node = (int*)(io + o_node);
        if (!empty) {
            voc_launch_transform(voc, st, f->desc, n, levelsup, d_word, d_leaf, d_node);
            CCM_HIP(c, hipGetLastError());
        }
        const bool on_device = n <= kBowDirMax;
        if (on_device) {
            // the launch overwrites the live directory before a step that can still fail: until the counts are back the handle has no bow
            f->has_bow = false;
            const BowDirArgs A{ n, empty ? nullptr : d_leaf, d_node, V.pos_dev, f->node, want && !empty ? d_node : nullptr, f->order, f->nodes,
                                f->first, d_cnt };
            if (bow_launch_directory(st, A)) return ccm_fail(c, CCM_E_DEVICE, "k_bow_directory: n = %d refused", n);
            CCM_HIP(c, hipGetLastError());
        }
        const bool fetch = !empty && (want || !on_device);
        if (on_device || fetch) { if ((rc = frame_download(c, fetch ? end : 16))) return rc; }
        const int32_t* h_word = (const int32_t*)(S.host + o_word); const int32_t* h_leaf = (const int32_t*)(S.host + o_leaf);
        const int32_t* h_node = (const int32_t*)(S.host + o_node);
        std::vector<int32_t> built;                                            // larger frames: the node per feature for the host build
        if (!on_device) {
            built.assign((size_t)std::max(n, 1), -1);
            if (!empty) for (int i = 0; i < n; i++) if (V.weight[h_leaf[i]] > 0) built[i] = h_node[i];
        }
        if (want) {
            for (int i = 0; i < n; i++) {
                word_id[i] = empty ? 0 : h_word[i];
                weight[i] = empty ? 0.0 : V.weight[h_leaf[i]];                 // m_nodes[final_id].weight (:1257)
                node[i] = empty ? -1 : on_device ? h_node[i] : built[i];
            }
        }
        if (!on_device) return bow_install(c, f, built.data(), "ccm_frame_compute_bow");
        int cnt[2];
        std::memcpy(cnt, S.host + o_cnt, 8);
        f->has_bow = true; f->n_bow = cnt[0]; f->n_nodes = cnt[1];
        return kf_gather(c, f);
    });
}

// KeyFrame::fx, fy, cx, cy, mvScaleFactors, mvLevelSigma2 (read by CreateNewMapPoints, src/Mapping.cpp:292-305, :337-349)
int ccm_frame_set_camera(ccm_frame* f, float fx, float fy, float cx, float cy, const float* scale_factors, const float* level_sigma2, int n_levels)
{
    if (!f) return CCM_E_ARG;
    ccm_ctx* c = f->ctx;
    if (!c) return CCM_E_STATE;
    return ccm_guard(c, "ccm_frame_set_camera", [&]() -> int {
        if (!scale_factors || !level_sigma2) return ccm_fail(c, CCM_E_ARG, "ccm_frame_set_camera: null %s", !scale_factors ? "scale_factors" : "level_sigma2");
        if (n_levels < f->n_levels || n_levels < 1 || n_levels > ccm_frame::kMaxLevels)
            return ccm_fail(c, CCM_E_ARG, "ccm_frame_set_camera: n_levels = %d outside [%d, %d]", n_levels, std::max(f->n_levels, 1), ccm_frame::kMaxLevels);
        CCM_HIP(c, hipSetDevice(c->device));
        int rc = kf_block(c, f);
        if (rc) return rc;
        // staged as [sf | sig2 | cam], which are neighbours in the block too (kf_layout): one copy, so a failure leaves nothing half written
        const size_t tab = ccm_frame::kMaxLevels * 4, end = 2 * tab + sizeof(MapCam);
        uint8_t* h = nullptr;
        if ((rc = frame_staging(c, end, &h))) return rc;
        std::memset(h, 0, 2 * tab);
        std::memcpy(h, scale_factors, (size_t)n_levels * 4); std::memcpy(h + tab, level_sigma2, (size_t)n_levels * 4);
        MapCam m = f->cam;
        m.fx = fx; m.fy = fy; m.cx = cx; m.cy = cy;
        m.invfx = 1.0f / fx; m.invfy = 1.0f / fy;                              // KeyFrame::invfx, invfy
        std::memcpy(h + 2 * tab, &m, sizeof(MapCam));
        if ((rc = frame_upload(c, 0, end, f->sf))) return rc;
        f->cam = m; f->has_cam = true; f->cam_levels = n_levels; f->sf1 = n_levels > 1 ? scale_factors[1] : 0.0f;
        return kf_gather(c, f);
    });
}

// KeyFrame::SetPose: Tcw and Ow as the keyframe stores them (GetRotation, GetTranslation, GetCameraCenter)
int ccm_frame_set_pose(ccm_frame* f, const float* Tcw, const float* Ow)
{
    if (!f) return CCM_E_ARG;
    ccm_ctx* c = f->ctx;
    if (!c) return CCM_E_STATE;
    return ccm_guard(c, "ccm_frame_set_pose", [&]() -> int {
        if (!Tcw || !Ow) return ccm_fail(c, CCM_E_ARG, "ccm_frame_set_pose: null %s", !Tcw ? "Tcw" : "Ow");
        CCM_HIP(c, hipSetDevice(c->device));
        int rc = kf_block(c, f);
        if (rc) return rc;
        uint8_t* h = nullptr;
        if ((rc = frame_staging(c, sizeof(MapCam), &h))) return rc;
        MapCam m = f->cam;
        std::memcpy(m.Tcw, Tcw, 48); std::memcpy(m.Ow, Ow, 12);
        std::memcpy(h, &m, sizeof(MapCam));
        if ((rc = frame_upload(c, 0, sizeof(MapCam), f->d_cam))) return rc;
        f->cam = m; f->has_pose = true;
        return CCM_OK;
    });
}

int ccm_frame_debug_bow(ccm_frame* f, int32_t* order, int32_t* nodes, int32_t* first)
{
    if (!f || !order || !nodes || !first) return CCM_E_ARG;
    ccm_ctx* c = f->ctx;
    if (!c) return CCM_E_STATE;
    if (!f->has_bow) return ccm_fail(c, CCM_E_STATE, "ccm_frame_debug_bow: no bow");
    CCM_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = frame_fetch(c, order, f->order, (size_t)f->n_bow * 4)) || (rc = frame_fetch(c, nodes, f->nodes, (size_t)f->n_nodes * 4)) ||
        (rc = frame_fetch(c, first, f->first, ((size_t)f->n_nodes + 1) * 4)))
        return rc;
    return f->n_nodes;
}

// ORBmatcher::SearchByProjection(Frame&, const vector<mpptr>&, th), ORBmatcher.cpp:71-148, frame side from the handle
int ccm_frame_search_by_projection(ccm_ctx* c, ccm_frame* f, const float* scale_factors, int n_mp, const uint8_t* in_view,
                                   const int32_t* level, const float* view_cos, const float* proj_x, const float* proj_y,
                                   const uint8_t* mp_desc, const uint8_t* mp_has_obs, const int32_t* query_mp_id,
                                   uint8_t* occupied, float th, float nnratio, int32_t* match)
{
    RoctxRange roctx_("ccm_frame_search_by_projection");
    if (!c || !f) return CCM_E_ARG;
    int rc = frame_check(c, f);
    if (rc) return rc;
    if (n_mp < 0 || (f->n > 0 && (!match || !occupied)) ||
        (n_mp > 0 && (!scale_factors || !in_view || !level || !view_cos || !proj_x || !proj_y || !mp_desc || !mp_has_obs)))
        return ccm_fail(c, CCM_E_ARG, "bad SearchByProjection arguments");
    for (int i = 0; i < f->n; i++) match[i] = -1;
    if (n_mp == 0 || f->n == 0) return 0;
    return ccm_guard(c, "ccm_frame_search_by_projection", [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        const WinQueries q = window_queries_projection(n_mp, in_view, level, view_cos, scale_factors, th);
        WinCall w{ 0, n_mp, proj_x, proj_y, q.qr.data(), q.minl.data(), q.maxl.data(), mp_desc, in_view, mp_has_obs, query_mp_id,
                   nullptr, nullptr, 0.f, nullptr, nnratio, 0, 0 };
        return frame_window(c, f, w, occupied, match);
    });
}

// ORBmatcher::SearchByProjection(Frame& Current, const Frame& Last, th), ORBmatcher.cpp:1350-1476, and the relocalisation
// overload (:1478-1605), current frame (and last frame) from handles
int ccm_frame_search_by_projection_frame(ccm_ctx* c, ccm_frame* cur, const ccm_frame* last, const float* scale_factors, int n_last,
                                         const uint8_t* valid, const float* u, const float* v, const int32_t* last_octave,
                                         const float* last_angle, const uint8_t* mp_desc, const uint8_t* mp_has_obs,
                                         const int32_t* query_mp_id, uint8_t* occupied, float th, int check_ori, int orb_dist,
                                         int32_t* match)
{
    RoctxRange roctx_("ccm_frame_search_by_projection_frame");
    if (!c || !cur) return CCM_E_ARG;
    int rc = frame_check(c, cur);
    if (rc || (last && (rc = frame_check(c, last)))) return rc;
    if (n_last < 0 || (last && n_last != last->n)) return ccm_fail(c, CCM_E_ARG, "n_last must be >= 0 and equal the last frame's N");
    if (check_ori && (!cur->has_angle || (last && !last->has_angle)))
        return ccm_fail(c, CCM_E_ARG, "orientation check against a frame created without angles");
    if ((cur->n > 0 && (!match || !occupied)) ||
        (n_last > 0 && (!scale_factors || !valid || !u || !v || !mp_desc || !mp_has_obs || (!last && (!last_octave || (check_ori && !last_angle))))))
        return ccm_fail(c, CCM_E_ARG, "bad SearchByProjection(frame, frame) arguments");
    for (int i = 0; i < cur->n; i++) match[i] = -1;
    if (n_last == 0 || cur->n == 0) return 0;
    return ccm_guard(c, "ccm_frame_search_by_projection_frame", [&]() -> int {
        CCM_HIP(c, hipSetDevice(c->device));
        WinQueries q;                                                          // a `last` handle: set up on the device
        if (!last) q = window_queries_frame(n_last, valid, last_octave, scale_factors, th);
        WinCall w{ 2, n_last, u, v, last ? nullptr : q.qr.data(), last ? nullptr : q.minl.data(), last ? nullptr : q.maxl.data(), mp_desc, valid,
                   mp_has_obs, query_mp_id, last, scale_factors, th, last_angle, 0.f, orb_dist, check_ori ? 1 : 0 };
        return frame_window(c, cur, w, occupied, match);
    });
}

// Optimizer::PoseOptimizationClient(Frame&), src/Optimizer.cpp:215-347, the frame's correspondences gathered on the device
int ccm_frame_pose_optimize(ccm_ctx* c, ccm_frame* f, int n_mp, const double* mp_xyz, const float* inv_level_sigma2, int n_levels,
                            const double intr[4], double pose7[7], uint8_t* outlier, int32_t* n_inliers)
{
    RoctxRange roctx_("ccm_frame_pose_optimize");
    if (!c || !f) return CCM_E_ARG;
    int rc = frame_check(c, f);
    if (rc) return rc;
    if (!intr || !pose7 || !n_inliers || n_mp < 0 || (n_mp > 0 && !mp_xyz) || (f->n > 0 && (!outlier || !inv_level_sigma2 || n_levels < 1)))
        return ccm_fail(c, CCM_E_ARG, "bad pose arguments");
    if (f->n == 0) { *n_inliers = 0; return CCM_OK; }
    return ccm_guard(c, "ccm_frame_pose_optimize", [&]() -> int {
        bool bad_id = false;
        if ((rc = frame_pose_run(c, f, n_mp, mp_xyz, nullptr, nullptr, inv_level_sigma2, n_levels, intr, pose7, outlier, n_inliers, &bad_id))) return rc;
        if (bad_id) return ccm_fail(c, CCM_E_ARG, "a map-point id outside [0, %d) or an octave outside [0, %d)", n_mp, n_levels);
        return CCM_OK;
    });
}

}  // extern "C"
