"""Frame handles built with the camera on the device (include/ccm_hot.h: ccm_frame_from_extract_camera, ccm_frames_from_extract_camera,
ccm_frame_get_keypoints): Frame::UndistortKeyPoints fused into the build kernel against the numpy restatement tests/undistort_ref.py
bit for bit, the grid on the undistorted coordinates, the old route (host undistortion + ccm_frame_from_extract) against the new one,
the early return, cropping bounds, the batched builder against the single call, and misuse.

Frames are synth.frame at 752 x 480.  Three kinds of extract: about 1000 keypoints (a few below the build kernel's 1024 threads, so
the last lanes of the gather idle and the grid's strided loops over 3600 cells take several rounds), fewer than 64 (one wave), and
none; the single-frame test adds 1500 and 5000 keypoints, where a thread of the gather takes a second keypoint and a second trip."""
import ctypes as C

import numpy as np
import pytest

import undistort_ref as R
from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.frame import Camera, DeviceFrame
from motioncheck_ccm_slam_amd.matcher import FRAME_GRID_COLS, FRAME_GRID_ROWS, FrameGridView, ORBmatcher
from motioncheck_ccm_slam_amd.orb import ORBextractor

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -7
W, H = 752, 480


def _flat():
    return np.full((H, W), 128, np.uint8)


def _patch():
    """A flat image with an 80 x 80 textured patch: a few dozen keypoints at 1000 features per image."""
    img = _flat()
    img[200:280, 300:380] = synth.frame(3, W, H)[200:280, 300:380]
    return img


# (extractor arguments, image): many, few (with 8 levels the quadtree's floor is 64 keypoints, so this one has 4), none
EXTRACTS = {"many": ((1000, 1.2, 8, 20, 7), lambda: synth.frame(0, W, H)),
            "few": ((10, 1.2, 4, 20, 7), lambda: synth.frame(1, W, H)),
            "none": ((1000, 1.2, 8, 20, 7), _flat),
            # beyond the issue's three: a second keypoint for some threads of the gather (n > 1024), and a second trip of its loop of
            # four keypoints per thread (n > 4096)
            "more": ((1500, 1.2, 8, 20, 7), lambda: synth.frame(0, W, H)),
            "most": ((5000, 1.2, 8, 20, 7), lambda: synth.frame(0, W, H))}


def _extract(ctx, kind):
    ex = ORBextractor(*EXTRACTS[kind][0], ctx=ctx)
    kps, desc = ex(EXTRACTS[kind][1]())
    assert {"many": 900 < len(kps) <= 1024, "few": 0 < len(kps) < 64, "none": len(kps) == 0, "more": 1024 < len(kps) <= 4096,
            "most": len(kps) > 4096}[kind], len(kps)
    return ex, kps, desc


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_xy(a, b):
    return len(a[0]) == len(b[0]) and (_bits(a[0]) == _bits(b[0])).all() and (_bits(a[1]) == _bits(b[1])).all()


def _round_half_away(v):
    t = np.trunc(v)
    return t + np.sign(v) * (np.abs(v - t) >= np.float32(0.5))


def _np_grid(kx, ky, b, cols=FRAME_GRID_COLS, rows=FRAME_GRID_ROWS):
    """Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cpp:103-118, 255-266) in float32 under the bounds b: cell k = px*rows + py,
    index order."""
    kx = np.asarray(kx, "f4"); ky = np.asarray(ky, "f4")
    fx = _round_half_away((kx - np.float32(b.min_x)) * np.float32(b.inv_w))
    fy = _round_half_away((ky - np.float32(b.min_y)) * np.float32(b.inv_h))
    ok = (fx >= 0) & (fx < cols) & (fy >= 0) & (fy < rows)
    cell = np.where(ok, fx.astype(np.int64) * rows + fy.astype(np.int64), -1)
    first = np.zeros(cols * rows + 1, "i4")
    np.add.at(first, cell[ok] + 1, 1)
    first = np.cumsum(first).astype("i4")
    idx = np.flatnonzero(ok)
    return first, idx[np.argsort(cell[ok], kind="stable")].astype("i4")


def _same_grid(a, b):
    return (a[0] == b[0]).all() and len(a[1]) == len(b[1]) and (a[1] == b[1]).all()


def _plain_bounds(min_x=0.0, max_x=float(W), min_y=0.0, max_y=float(H)):
    return _lib.FrameBounds(min_x, max_x, min_y, max_y, float(np.float32(FRAME_GRID_COLS) / np.float32(max_x - min_x)),
                            float(np.float32(FRAME_GRID_ROWS) / np.float32(max_y - min_y)))


def _map_points(kx, ky, octave, desc, seed, n_true=1200, n_rand=300):
    """Map points re-projected with noise from the frame's own features, plus unrelated ones (as tests/test_frame_gpu.py)."""
    n = len(kx)
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, n_true)
    flips = np.packbits(rng.random((n_true, 256)) < 0.05, axis=1, bitorder="little")
    nm = n_true + n_rand
    return dict(
        mp_desc=np.concatenate([desc[src] ^ flips, rng.integers(0, 256, (n_rand, 32), dtype=np.uint8)]),
        px=np.concatenate([kx[src] + rng.normal(0, 1.5, n_true), rng.uniform(0, W, n_rand)]).astype("f4"),
        py=np.concatenate([ky[src] + rng.normal(0, 1.5, n_true), rng.uniform(0, H, n_rand)]).astype("f4"),
        level=np.concatenate([np.clip(octave[src] + rng.integers(0, 2, n_true), 0, 7), rng.integers(0, 8, n_rand)]).astype("i4"),
        view_cos=rng.uniform(0.99, 1.0, nm).astype("f4"), in_view=rng.random(nm) < 0.9, has_obs=rng.random(nm) < 0.95,
        occupied=rng.random(n) < 0.2)


def _search(m, h, sf, mp):
    return m.SearchByProjectionHandle(h, sf, mp["in_view"], mp["level"], mp["view_cos"], mp["px"], mp["py"], mp["mp_desc"], mp["has_obs"],
                                      mp["occupied"], 3.0)


def _same_search(a, b):
    return a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all()


# ---------------------------------------------------------------------------------------------------------------- 1. single frame
@pytest.mark.parametrize("kind", ["many", "few", "none", "more", "most"])
@pytest.mark.parametrize("cam_name", ["euroc", "synthetic"])
def test_single_frame_matches_the_restatement(ctx, kind, cam_name):
    camd = {"euroc": R.EUROC, "synthetic": R.SYNTH}[cam_name]
    cam = Camera(**camd)
    b = cam.image_bounds(W, H)
    ex, kps, desc = _extract(ctx, kind)
    with DeviceFrame.from_extract(ex, 0, camera=cam, bounds=b, ctx=ctx) as h:
        assert h.n == len(kps)
        got = h.keypoints()
        want = R.undistort(camd, kps["x"], kps["y"])
        assert _same_xy(got, want)
        assert _same_xy(got, cam.undistort(kps["x"], kps["y"]))    # host and device: one arithmetic, two compilers
        assert _same_grid(h.grid(), _np_grid(want[0], want[1], b))
        assert (h.map_points == -1).all()
        if kind == "many":
            first = h.grid()[0]
            assert first[-1] == h.n and (np.diff(first) > 1).sum() > 20   # nothing leaves the image bounds; the in-cell order is exercised
            assert np.abs(got[0] - kps["x"]).max() > 1.0


# ---------------------------------------------------------------------------------------------------------------- 2. old route = new route
def test_old_route_equals_new_route(ctx):
    cam = Camera(**R.EUROC)
    b = cam.image_bounds(W, H)
    ex, kps, desc = _extract(ctx, "many")
    sf = ex.GetScaleFactors()
    kxu, kyu = cam.undistort(kps["x"], kps["y"])                   # today's route: host undistortion, arrays uploaded
    h_old = DeviceFrame.from_extract(ex, 0, kxu, kyu, min_x=b.min_x, max_x=b.max_x, min_y=b.min_y, max_y=b.max_y, ctx=ctx)
    h_new = DeviceFrame.from_extract(ex, 0, camera=cam, bounds=b, ctx=ctx)
    try:
        assert h_old.n == h_new.n == len(kps)
        ko, kn = h_old.keypoints(), h_new.keypoints()
        assert ko[0].tobytes() == kn[0].tobytes() and ko[1].tobytes() == kn[1].tobytes()
        go, gn = h_old.grid(), h_new.grid()
        assert go[0].tobytes() == gn[0].tobytes() and go[1].tobytes() == gn[1].tobytes()
        mp = _map_points(kxu, kyu, kps["octave"], desc, 2)
        m = ORBmatcher(0.8, ctx=ctx)
        ro, rn = _search(m, h_old, sf, mp), _search(m, h_new, sf, mp)
        assert ro[0] == rn[0] and ro[1].tobytes() == rn[1].tobytes() and ro[2].tobytes() == rn[2].tobytes()
        assert ro[0] > 300                                         # not a comparison of empty results
        assert (h_old.map_points == h_new.map_points).all()
        # and the host-buffer matcher on the restated coordinates agrees (descriptors and octaves were gathered as before)
        view = FrameGridView(kxu, kyu, kps["octave"], desc, b.min_x, b.max_x, b.min_y, b.max_y)
        ref = m.SearchByProjection(view, sf, mp["in_view"], mp["level"], mp["view_cos"], mp["px"], mp["py"], mp["mp_desc"], mp["has_obs"],
                                   mp["occupied"], 3.0)
        assert _same_search(ref, rn)
    finally:
        h_old.close(); h_new.close()


# ---------------------------------------------------------------------------------------------------------------- 3. early return
def test_early_return_keeps_the_extracted_coordinates(ctx):
    ex, kps, desc = _extract(ctx, "many")
    with DeviceFrame.from_extract(ex, 0, ctx=ctx) as plain:
        want_xy, want_grid = plain.keypoints(), plain.grid()
    assert _same_xy(want_xy, (kps["x"], kps["y"]))
    k1_zero = Camera(**R.K1_ZERO)                                   # k1 == 0 with k2, p1, p2, k3 set
    for cam, b in ((k1_zero, k1_zero.image_bounds(W, H)), (None, _plain_bounds())):
        with DeviceFrame.from_extract(ex, 0, camera=cam, bounds=b, ctx=ctx) as h:
            assert h.n == len(kps) and _same_xy(h.keypoints(), want_xy) and _same_grid(h.grid(), want_grid)
            assert (h.map_points == -1).all()


# ---------------------------------------------------------------------------------------------------------------- 4. cropping bounds
def test_bounds_narrower_than_the_undistorted_extent(ctx):
    cam = Camera(**R.EUROC)
    ex, kps, desc = _extract(ctx, "many")
    b = _plain_bounds()                                            # 0, 752, 0, 480: the undistorted image is larger
    with DeviceFrame.from_extract(ex, 0, camera=cam, bounds=b, ctx=ctx) as h:
        want = R.undistort(R.EUROC, kps["x"], kps["y"])
        assert _same_xy(h.keypoints(), want)
        first, items = h.grid()
        assert _same_grid((first, items), _np_grid(want[0], want[1], b))
        assert first[-1] < h.n                                     # features whose undistorted position leaves the grid get no cell
        outside = (want[0] < -1) | (want[0] > W + 11) | (want[1] < -1) | (want[1] > H + 11)
        assert outside.any() and not np.isin(np.flatnonzero(outside), items).any()


# ---------------------------------------------------------------------------------------------------------------- 5. batch
@pytest.mark.parametrize("with_camera", [True, False])
def test_batch_equals_single_calls(ctx, with_camera):
    cam = Camera(**R.EUROC) if with_camera else None
    b = cam.image_bounds(W, H) if with_camera else _plain_bounds()
    imgs = np.stack([synth.frame(0, W, H), synth.frame(1, W, H), _patch(), _flat(), synth.frame(2, W, H)])
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    kps, desc, counts = ex.extract_batch(imgs)
    first_image, count = 1, 4                                      # many, few, none, many
    ns = [int(c) for c in counts[first_image:first_image + count]]
    assert ns[0] > 900 and 0 < ns[1] < 64 and ns[2] == 0 and ns[3] > 900, ns
    sf = ex.GetScaleFactors()
    m = ORBmatcher(0.8, ctx=ctx)
    batch = DeviceFrame.batch_from_extract(ex, first_image, count, cam, b, ctx=ctx)
    singles = [DeviceFrame.from_extract(ex, first_image + k, camera=cam, bounds=b, ctx=ctx) for k in range(count)]
    kept = []
    try:
        assert len(batch) == count
        for k, (hb, hs) in enumerate(zip(batch, singles)):
            img = first_image + k
            kp = kps[img, :ns[k]]
            assert hb.n == hs.n == ns[k]
            xy = hb.keypoints()
            assert _same_xy(xy, hs.keypoints())
            assert _same_xy(xy, R.undistort(R.EUROC, kp["x"], kp["y"]) if with_camera else (kp["x"], kp["y"]))
            g = hb.grid()
            assert _same_grid(g, hs.grid()) and _same_grid(g, _np_grid(xy[0], xy[1], b))
            assert (hb.map_points == -1).all() and (hs.map_points == -1).all()
            res = None
            if ns[k] > 0:
                mp = _map_points(xy[0], xy[1], kp["octave"], desc[img, :ns[k]], 10 + k)
                res = _search(m, hb, sf, mp)
                assert _same_search(res, _search(m, hs, sf, mp)) and (hb.map_points == hs.map_points).all()
                assert res[0] > (300 if ns[k] > 900 else 0)
                hb.map_points = None
            kept.append((xy, g, mp if ns[k] > 0 else None, res))
        # a later extract on the same context: the handles own their data
        ex.extract_batch(imgs[::-1].copy())
        for hb, (xy, g, mp, res) in zip(batch, kept):
            assert _same_xy(hb.keypoints(), xy) and _same_grid(hb.grid(), g)
            if mp is not None:
                assert _same_search(_search(m, hb, sf, mp), res)
    finally:
        for h in batch + singles:
            h.close()
    # the blocks went back to the pool: a second batch of the same shape (now of the reversed extract) succeeds and is right
    again = DeviceFrame.batch_from_extract(ex, 0, count, cam, b, ctx=ctx)
    try:
        for k, h in enumerate(again):
            kp = kps[4 - k, :int(counts[4 - k])]
            assert h.n == len(kp)
            assert _same_xy(h.keypoints(), R.undistort(R.EUROC, kp["x"], kp["y"]) if with_camera else (kp["x"], kp["y"]))
    finally:
        for h in again:
            h.close()
    assert DeviceFrame.batch_from_extract(ex, 2, 0, cam, b, ctx=ctx) == []      # n_images == 0 is OK


# ---------------------------------------------------------------------------------------------------------------- 6. errors
def test_misuse_returns_error_codes(ctx):
    lib = _lib.load()
    cam = Camera(**R.EUROC)
    b = cam.image_bounds(W, H)
    cs, bs = C.byref(cam.struct), C.byref(b)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
    ex.extract_batch(np.stack([synth.frame(0, W, H), _patch()]))
    h = C.c_void_p(77)
    outs = (C.c_void_p * 3)(1, 2, 3)

    def cleared(count):
        """out[0 .. count) is all NULL; the entries are then made non-NULL again for the next call."""
        got = [outs[k] for k in range(max(count, 0))]
        for k in range(3):
            outs[k] = k + 1
        return all(g is None for g in got)

    other = _lib.Context(0)
    try:
        # no extract on this context yet
        assert lib.ccm_frame_from_extract_camera(other.handle, 0, -1, cs, bs, 75, 48, C.byref(h)) == E_STATE and h.value is None
        assert lib.ccm_frames_from_extract_camera(other.handle, 0, 1, cs, bs, 75, 48, outs) == E_STATE and cleared(1)
        # the image range
        for image in (-1, 2):
            assert lib.ccm_frame_from_extract_camera(ctx.handle, image, -1, cs, bs, 75, 48, C.byref(h)) == E_ARG and h.value is None
        for first, count in ((-1, 2), (0, 3), (1, 2), (2, 1), (0, -1)):
            assert lib.ccm_frames_from_extract_camera(ctx.handle, first, count, cs, bs, 75, 48, outs) == E_ARG and cleared(count), (first, count)
        # n above the extract's max_per_image
        assert lib.ccm_frame_from_extract_camera(ctx.handle, 0, ex.max_per_image + 1, cs, bs, 75, 48, C.byref(h)) == E_ARG
        assert lib.ccm_frame_from_extract_camera(ctx.handle, 0, -2, cs, bs, 75, 48, C.byref(h)) == E_ARG
        # bounds, focal length, grid
        assert lib.ccm_frame_from_extract_camera(ctx.handle, 0, -1, cs, None, 75, 48, C.byref(h)) == E_ARG
        assert lib.ccm_frames_from_extract_camera(ctx.handle, 0, 2, None, None, 75, 48, outs) == E_ARG and cleared(2)
        bad = Camera(**dict(R.EUROC, fy=0.0))
        assert lib.ccm_frame_from_extract_camera(ctx.handle, 0, -1, C.byref(bad.struct), bs, 75, 48, C.byref(h)) == E_ARG
        assert lib.ccm_frames_from_extract_camera(ctx.handle, 0, 2, C.byref(bad.struct), bs, 75, 48, outs) == E_ARG and cleared(2)
        assert lib.ccm_frame_from_extract_camera(ctx.handle, 0, -1, cs, bs, 0, 48, C.byref(h)) == E_ARG
        assert lib.ccm_frames_from_extract_camera(ctx.handle, 0, 2, cs, bs, 75, 48, None) == E_ARG
        # a handle that outlived its context
        ORBextractor(1000, 1.2, 8, 20, 7, ctx=other).extract_batch(_patch()[None])
        f = DeviceFrame.from_extract(None, 0, camera=cam, bounds=b, ctx=other)
        kx = np.zeros(max(f.n, 1), "f4")
        assert f.n > 0 and lib.ccm_frame_get_keypoints(C.c_void_p(f.handle), _lib.ptr(kx), None) == 0
        other.close()
        assert lib.ccm_frame_get_keypoints(C.c_void_p(f.handle), _lib.ptr(kx), _lib.ptr(kx)) == E_STATE
        f.close()
    finally:
        other.close()
    # after all that the context still builds handles
    with DeviceFrame.from_extract(ex, 1, camera=cam, bounds=b, ctx=ctx) as ok:
        assert 0 < ok.n < 64
