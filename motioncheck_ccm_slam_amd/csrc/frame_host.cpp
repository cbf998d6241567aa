// frame_host.cpp -- C ABI of the frame handles (include/ccm_hot.h "frame handles"): one Frame's features, descriptors, grid and
// map-point ids in device memory, reused by the per-frame matchers (frame_window_host.cpp) and the pose optimisation
// (frame_pose_host.cpp) of Tracking.  Here: the handles' lifetime and block pools, the setters, the keyframe part, ComputeBoW and the
// debug taps.  Every setter stages its arrays in the context's block (staging.h) in the layout of their destination and sends them
// with one copy; ComputeBoW stages [ counts | word | leaf | node ] down and uploads nothing.  The camera calls (Frame::UndistortKeyPoints,
// Frame::ComputeImageBounds on the host from undistort.h; the handles of one or many extracted images with the undistortion done in
// k_frame_build_batch) stage one record per frame.
#include "frame_internal.h"
#include "bow_directory.h"
#include <algorithm>
#include <cstdarg>

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
    S->stage.release();
    delete S;
    c->frame = nullptr;
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
int kf_block(ccm_ctx* c, ccm_frame* f)
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
    Staging& G = frame_state(c)->stage;
    if ((rc = G.reserve(c, L.bow_end))) return rc;
    G.put(L.node, node, (size_t)n * 4);
    G.put(L.order, D.order.data(), D.order.size() * 4);
    G.put(L.nodes, D.nodes.data(), D.nodes.size() * 4);
    G.put(L.first, D.first.data(), D.first.size() * 4);
    // the copy is queued over the live directory before the event record that can still fail: then the handle has no bow at all
    if ((rc = G.upload(c, 0, L.bow_end, f->kf_mem->buf.p))) { f->has_bow = false; return rc; }
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

int frame_named_check(ccm_ctx* c, const ccm_frame* f, int orphaned, const char* fn, const char* who, ...)
{
    if (f && f->ctx == c) return CCM_OK;         // the name is made only for a message
    char name[48];
    va_list ap;
    va_start(ap, who);
    vsnprintf(name, sizeof name, who, ap);
    va_end(ap);
    if (!f) return ccm_fail(c, CCM_E_ARG, "%s: %s is null", fn, name);
    if (!f->ctx) return ccm_fail(c, orphaned, "%s: %s outlived its context", fn, name);
    if (f->ctx != c) return ccm_fail(c, CCM_E_ARG, "%s: %s belongs to another context", fn, name);
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
        Staging& G = frame_state(c)->stage;
        int rc = G.reserve(c, L.upload_end);
        if (rc) return rc;
        G.put(L.kx, g->kp_x, (size_t)n * 4); G.put(L.ky, g->kp_y, (size_t)n * 4);
        G.put(L.oct, g->kp_octave, (size_t)n * 4);
        if (angle) G.put(L.angle, angle, (size_t)n * 4);
        else std::memset(G.host<float>(L.angle), 0, (size_t)n * 4);
        G.put(L.desc, g->desc, (size_t)n * 32);
        ccm_frame* f = nullptr;
        if ((rc = frame_alloc(c, n, g->grid_cols, g->grid_rows, &f))) return rc;
        f->n_levels = max_oct + 1; f->has_angle = angle != nullptr;
        f->min_x = g->min_x; f->min_y = g->min_y; f->inv_w = g->inv_w; f->inv_h = g->inv_h;
        if ((rc = G.upload(c, 0, L.upload_end, f->mem->buf.p)) || (rc = frame_build(c, f, nullptr, nullptr, 0))) { frame_release(f); return rc; }
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
        Staging& G = frame_state(c)->stage;
        if (kp_x_un) {
            if ((rc = G.reserve(c, L.oct))) return rc;
            G.put(L.kx, kp_x_un, (size_t)n * 4); G.put(L.ky, kp_y_un, (size_t)n * 4);
        }
        ccm_frame* f = nullptr;
        if ((rc = frame_alloc(c, n, grid_cols, grid_rows, &f))) return rc;
        f->n_levels = nlevels; f->has_angle = true;
        f->min_x = min_x; f->min_y = min_y; f->inv_w = inv_w; f->inv_h = inv_h;
        if ((kp_x_un && (rc = G.upload(c, 0, L.oct, f->mem->buf.p))) ||
            (rc = frame_build(c, f, kps + (size_t)image * max_per_image, desc + (size_t)image * max_per_image * 32, kp_x_un ? 1 : 0))) {
            frame_release(f); return rc;
        }
        *out = f;
        return CCM_OK;
    });
}

int ccm_undistort_points(const ccm_camera* cam, int n, const float* x, const float* y, float* x_un, float* y_un)
{
    if (!cam || n < 0 || (n > 0 && (!x || !y || !x_un || !y_un)) || cam->fx == 0.0f || cam->fy == 0.0f) return CCM_E_ARG;
    if (cam->k1 == 0.0f) {                                                       // mvKeysUn = mvKeys (:279-283)
        if (n && x_un != x) std::memmove(x_un, x, (size_t)n * 4);
        if (n && y_un != y) std::memmove(y_un, y, (size_t)n * 4);
        return CCM_OK;
    }
    const UndistortCam U = undistort_cam(*cam);
    for (int i = 0; i < n; i++) undistort_point(U, x[i], y[i], &x_un[i], &y_un[i]);
    return CCM_OK;
}

int ccm_image_bounds(const ccm_camera* cam, int width, int height, int grid_cols, int grid_rows, ccm_frame_bounds* out)
{
    if (!cam || !out || width < 1 || height < 1 || grid_cols < 1 || grid_rows < 1 || cam->fx == 0.0f || cam->fy == 0.0f) return CCM_E_ARG;
    ccm_frame_bounds b;
    if (cam->k1 != 0.0f) {                                                       // the corners in the order of :314-317
        float cx[4] = { 0.0f, (float)width, 0.0f, (float)width }, cy[4] = { 0.0f, 0.0f, (float)height, (float)height };
        const UndistortCam U = undistort_cam(*cam);
        for (int i = 0; i < 4; i++) undistort_point(U, cx[i], cy[i], &cx[i], &cy[i]);
        b.min_x = std::min(cx[0], cx[2]); b.max_x = std::max(cx[1], cx[3]);
        b.min_y = std::min(cy[0], cy[1]); b.max_y = std::max(cy[2], cy[3]);
    } else {
        b.min_x = 0.0f; b.max_x = (float)width; b.min_y = 0.0f; b.max_y = (float)height;
    }
    b.inv_w = (float)grid_cols / (b.max_x - b.min_x);                            // :87-88
    b.inv_h = (float)grid_rows / (b.max_y - b.min_y);
    *out = b;
    return CCM_OK;
}

// The two calls below: n_images handles from consecutive images of the last extract through one launch of k_frame_build_batch.
// n >= 0 is the caller's count of a single image; n < 0 reads the counts of the range with one fetch.
static int frames_from_extract(ccm_ctx* c, const char* fn, int first_image, int n_images, int n, const ccm_camera* cam,
                               const ccm_frame_bounds* b, int grid_cols, int grid_rows, ccm_frame** out)
{
    if (!b || !grid_ok(grid_cols, grid_rows)) return ccm_fail(c, CCM_E_ARG, "%s: bad frame arguments (bounds, grid of at most 16384 cells)", fn);
    if (cam && (cam->fx == 0.0f || cam->fy == 0.0f)) return ccm_fail(c, CCM_E_ARG, "%s: zero focal length", fn);
    std::vector<ccm_frame*> made;
    const int rc = ccm_guard(c, fn, [&]() -> int {
        const ccm_keypoint* kps = nullptr; const uint8_t* desc = nullptr; const int32_t* counts = nullptr;
        int have = 0, max_per_image = 0, nlevels = 0;
        int rc = orb_last_result(c, &kps, &desc, &counts, &have, &max_per_image, &nlevels);
        if (rc) return rc;
        if (first_image < 0 || n_images < 0 || first_image > have || n_images > have - first_image || (n >= 0 && first_image >= have))
            return ccm_fail(c, CCM_E_ARG, "%s: images [%d, %d + %d) out of range [0, %d)", fn, first_image, first_image, n_images, have);
        if (n > max_per_image) return ccm_fail(c, CCM_E_ARG, "%s: n %d above the extract's max_per_image %d", fn, n, max_per_image);
        if (n_images == 0) return CCM_OK;
        CCM_HIP(c, hipSetDevice(c->device));
        std::vector<int32_t> cnt((size_t)n_images, n);
        if (n < 0) {
            if ((rc = frame_fetch(c, cnt.data(), counts + first_image, (size_t)n_images * 4))) return rc;
            for (int32_t& v : cnt) v = std::max(0, std::min<int>(v, max_per_image));
        }
        Staging& G = frame_state(c)->stage;
        const size_t end = (size_t)n_images * sizeof(FrameBatchRec);
        if ((rc = G.reserve(c, end))) return rc;
        FrameBatchRec* rec = G.host<FrameBatchRec>(0);
        made.reserve((size_t)n_images);
        for (int k = 0; k < n_images; k++) {
            ccm_frame* f = nullptr;
            if ((rc = frame_alloc(c, cnt[k], grid_cols, grid_rows, &f))) return rc;
            made.push_back(f);
            f->n_levels = nlevels; f->has_angle = true;
            f->min_x = b->min_x; f->min_y = b->min_y; f->inv_w = b->inv_w; f->inv_h = b->inv_h;
            const size_t row = (size_t)(first_image + k) * max_per_image;
            rec[k] = FrameBatchRec{ kps + row, desc + row * 32, f->n, 0, f->kx, f->ky, f->oct, f->angle, f->desc, f->cell_first, f->cell_items,
                                    f->mp_id };
        }
        if ((rc = G.upload(c, 0, end))) return rc;
        FrameBatchArgs A{};
        A.rec = G.dev<FrameBatchRec>(0);
        A.cols = grid_cols; A.rows = grid_rows; A.min_x = b->min_x; A.min_y = b->min_y; A.inv_w = b->inv_w; A.inv_h = b->inv_h;
        A.undistort = cam && cam->k1 != 0.0f;                                  // the early return of :279-283
        if (A.undistort) A.cam = undistort_cam(*cam);
        if (frame_launch_build_batch(c->stream, n_images, A)) return ccm_fail(c, CCM_E_DEVICE, "k_frame_build_batch: LDS request refused");
        CCM_HIP(c, hipGetLastError());
        return CCM_OK;
    });
    if (rc) { for (ccm_frame* f : made) frame_release(f); return rc; }
    for (size_t k = 0; k < made.size(); k++) out[k] = made[k];
    return CCM_OK;
}

int ccm_frame_from_extract_camera(ccm_ctx* c, int image, int n, const ccm_camera* cam, const ccm_frame_bounds* b, int grid_cols,
                                  int grid_rows, ccm_frame** out)
{
    RoctxRange roctx_("ccm_frame_from_extract_camera");
    if (out) *out = nullptr;
    if (!c || !out) return CCM_E_ARG;
    if (n < -1) return ccm_fail(c, CCM_E_ARG, "ccm_frame_from_extract_camera: n = %d", n);
    return frames_from_extract(c, "ccm_frame_from_extract_camera", image, 1, n, cam, b, grid_cols, grid_rows, out);
}

int ccm_frames_from_extract_camera(ccm_ctx* c, int first_image, int n_images, const ccm_camera* cam, const ccm_frame_bounds* b,
                                   int grid_cols, int grid_rows, ccm_frame** out)
{
    RoctxRange roctx_("ccm_frames_from_extract_camera");
    if (out) for (int k = 0; k < n_images; k++) out[k] = nullptr;
    if (!c || (!out && n_images != 0)) return CCM_E_ARG;
    return frames_from_extract(c, "ccm_frames_from_extract_camera", first_image, n_images, -1, cam, b, grid_cols, grid_rows, out);
}

int ccm_frame_get_keypoints(ccm_frame* f, float* kx, float* ky)
{
    if (!f) return CCM_E_ARG;
    ccm_ctx* c = f->ctx;
    if (!c) return CCM_E_STATE;
    CCM_HIP(c, hipSetDevice(c->device));
    int rc = kx ? frame_fetch(c, kx, f->kx, (size_t)f->n * 4) : CCM_OK;
    if (rc || !ky) return rc;
    return frame_fetch(c, ky, f->ky, (size_t)f->n * 4);
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
        Staging& G = frame_state(c)->stage;
        int rc = G.reserve(c, (size_t)f->n * 4);
        if (rc) return rc;
        G.put(0, mp_id, (size_t)f->n * 4);
        return G.upload(c, 0, (size_t)f->n * 4, f->mp_id);
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
        Staging& G = frame_state(c)->stage;
        hipStream_t st = c->stream;
        const int n = f->n;
        const bool empty = V.n_words == 0;                                     // empty(): transform() returns nothing (:1133)
        size_t off = 0;
        const size_t o_cnt = seg(off, 16), o_word = seg(off, (size_t)n * 4), o_leaf = seg(off, (size_t)n * 4), o_node = seg(off, (size_t)n * 4);
        const size_t end = off;
        if ((rc = G.reserve(c, end)) || (rc = kf_block(c, f))) return rc;
        int* d_cnt = G.dev<int>(o_cnt); int* d_word = G.dev<int>(o_word); int* d_leaf = G.dev<int>(o_leaf); int* d_node = G.dev<int>(o_node);
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
        if ((on_device || fetch) && ((rc = G.download(c, 0, fetch ? end : 16)) || (rc = G.wait(c)))) return rc;
        const int32_t* h_word = G.host<int32_t>(o_word); const int32_t* h_leaf = G.host<int32_t>(o_leaf);
        const int32_t* h_node = G.host<int32_t>(o_node);
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
        G.get(cnt, o_cnt, 8);
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
        Staging& G = frame_state(c)->stage;
        if ((rc = G.reserve(c, end))) return rc;
        std::memset(G.host<float>(0), 0, 2 * tab);
        G.put(0, scale_factors, (size_t)n_levels * 4); G.put(tab, level_sigma2, (size_t)n_levels * 4);
        MapCam m = f->cam;
        m.fx = fx; m.fy = fy; m.cx = cx; m.cy = cy;
        m.invfx = 1.0f / fx; m.invfy = 1.0f / fy;                              // KeyFrame::invfx, invfy
        G.put(2 * tab, &m, sizeof(MapCam));
        if ((rc = G.upload(c, 0, end, f->sf))) return rc;
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
        Staging& G = frame_state(c)->stage;
        if ((rc = G.reserve(c, sizeof(MapCam)))) return rc;
        MapCam m = f->cam;
        std::memcpy(m.Tcw, Tcw, 48); std::memcpy(m.Ow, Ow, 12);
        G.put(0, &m, sizeof(MapCam));
        if ((rc = G.upload(c, 0, sizeof(MapCam), f->d_cam))) return rc;
        f->cam = m; f->has_pose = true;
        return CCM_OK;
    });
}

// Test tap: Tcw and Ow as the DEVICE holds them (ccm_frame_set_pose uploads them, ccm_ba_solve_table_frames writes them there)
int ccm_frame_get_pose(ccm_frame* f, float* Tcw, float* Ow)
{
    if (!f || !Tcw || !Ow) return CCM_E_ARG;
    ccm_ctx* c = f->ctx;
    if (!c) return CCM_E_STATE;
    return ccm_guard(c, "ccm_frame_get_pose", [&]() -> int {
        if (!f->has_pose || !f->d_cam) return ccm_fail(c, CCM_E_STATE, "ccm_frame_get_pose: no pose");
        CCM_HIP(c, hipSetDevice(c->device));
        MapCam m;
        int rc = frame_fetch(c, &m, f->d_cam, sizeof(MapCam));
        if (rc) return rc;
        std::memcpy(Tcw, m.Tcw, 48); std::memcpy(Ow, m.Ow, 12);
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

}  // extern "C"
