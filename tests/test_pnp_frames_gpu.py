"""ccm_pnp_solver_create_frames on the GPU: the PnP correspondences gathered by k_pnp_gather from a frame handle and the map-point
table against the same solvers created from host arrays (ccm_pnp_solver_create), with the same draws.  Both routes run the same two
solver kernels, so every stored array must agree bit for bit; the arrays of the second route are the restatement of the
constructor's loop in tests/relocalization_ref.py.

Shapes: one frame of 90 features and three candidates of 12, 64 and 70 correspondences (one mask word exactly, and one past it); the
gather launch is one workgroup of 256 threads, of which 146 have a correspondence."""
import ctypes as C

import numpy as np
import pytest

import relocalization_ref as RR
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.matcher import FrameGridView
from motioncheck_ccm_slam_amd.pnpsolver import PnPSolver, make_draws
from motioncheck_ccm_slam_amd.tracking import MapPointTable
import pnp_solver_ref as P

pytestmark = pytest.mark.gpu
E_ARG = -1
N_CUR, SIZES, N_LEVELS = 90, (12, 64, 70), 8
MAX_ITS, RESERVE = 40, 5
SIGMA2 = (np.float32(1.2) ** (2 * np.arange(N_LEVELS))).astype("f4")


def _scene(seed=3):
    """A frame of N_CUR keypoints and, per candidate, a pose and points that project onto a subset of them (30 % wrong matches).
    Slot 0 is not LIVE, slot 1 is BAD and LIVE; the candidates' points follow."""
    rng = np.random.default_rng(seed)
    kx = rng.uniform(20, 620, N_CUR).astype("f4"); ky = rng.uniform(20, 460, N_CUR).astype("f4")
    octave = rng.integers(0, N_LEVELS, N_CUR).astype("i4")
    cap = 2 + sum(SIZES) + 3
    pos = np.zeros((cap, 3), "f4"); flags = np.zeros(cap, np.uint8)
    flags[1] = _lib.MP_LIVE | _lib.MP_BAD; pos[1] = (1, 2, 3)
    Ks, mp_ids, base = [], [], 2
    for n in SIZES:
        K = np.array([520.0 + rng.uniform(-20, 20), 520.0 + rng.uniform(-20, 20), 320.0 + rng.uniform(-8, 8), 240.0 + rng.uniform(-8, 8)])
        Rm = P._rotation(rng, rng.uniform(0.1, 1.2)); t = rng.uniform(-2, 2, 3)
        feat = np.sort(rng.choice(N_CUR, n, replace=False))
        uv = np.stack([kx[feat], ky[feat]], 1).astype("f8") + rng.normal(0, 0.5, (n, 2))
        wrong = rng.random(n) < 0.3
        uv[wrong] = np.stack([rng.uniform(0, 640, int(wrong.sum())), rng.uniform(0, 480, int(wrong.sum()))], 1)
        z = rng.uniform(2, 10, n)
        Xc = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], 1)
        slots = base + np.arange(n)
        pos[slots] = ((Xc - t) @ Rm).astype("f4"); flags[slots] = _lib.MP_LIVE | _lib.MP_HAS_OBS
        ids = np.full(N_CUR, -1, "i4"); ids[feat] = slots
        Ks.append(K.astype("f4")); mp_ids.append(ids); base += n
    return dict(kx=kx, ky=ky, oct=octave, desc=rng.integers(0, 256, (N_CUR, 32)).astype(np.uint8), pos=pos, flags=flags, K=np.array(Ks, "f4"),
                mp_id=mp_ids, cap=cap)


def _correspondences(S):
    """Per candidate, what the caller of either route collects: the features that hold a point which is not bad, in feature order."""
    usable = (S["flags"] & _lib.MP_BAD) == 0
    per = [RR.pnp_correspondences(S["kx"], S["ky"], S["oct"], SIGMA2, ids, S["pos"], usable) for ids in S["mp_id"]]
    first = np.concatenate([[0], np.cumsum([len(p[3]) for p in per])]).astype("i4")
    cat = lambda j: np.concatenate([p[j] for p in per])
    slot = np.concatenate([ids[p[3]] for ids, p in zip(S["mp_id"], per)]).astype("i4")
    return dict(first=first, P2D=cat(0), P3Dw=cat(1), sigma2=cat(2), feature=cat(3).astype("i4"), slot=slot)


@pytest.fixture(scope="module")
def world(ctx):
    S = _scene()
    Cq = _correspondences(S)
    assert tuple(np.diff(Cq["first"])) == SIZES
    draws = make_draws(np.random.default_rng(5), SIZES, MAX_ITS + RESERVE)
    t = MapPointTable(S["cap"], ctx=ctx)
    z3 = np.zeros((S["cap"], 3), "f4"); z1 = np.zeros(S["cap"], "f4")
    t.update(np.arange(S["cap"]), pos=S["pos"], normal=z3, min_dist=z1, max_dist=z1, desc=np.zeros((S["cap"], 32), np.uint8), flags=S["flags"])
    cur = DeviceFrame(FrameGridView(S["kx"], S["ky"], S["oct"], S["desc"]), np.zeros(N_CUR, "f4"), ctx=ctx)
    yield dict(S=S, Cq=Cq, draws=draws, table=t, cur=cur)
    cur.close(); t.close()


def _by_arrays(ctx, W):
    Cq = W["Cq"]
    s = PnPSolver(Cq["first"], np.full(len(SIZES), N_CUR, "i4"), W["S"]["K"], Cq["P2D"], Cq["P3Dw"], Cq["sigma2"], Cq["feature"], W["draws"],
                  reserve=RESERVE, detail=True, ctx=ctx)
    s.SetRansacParameters(0.99, 8, MAX_ITS, 4, 0.4, 5.991)
    return s


def _by_frames(ctx, W, feature=None, slot=None, level_sigma2=SIGMA2):
    Cq = W["Cq"]
    s = PnPSolver.from_frames(W["cur"], W["table"], Cq["first"], W["S"]["K"], Cq["feature"] if feature is None else feature,
                              Cq["slot"] if slot is None else slot, level_sigma2, W["draws"], reserve=RESERVE, detail=True, ctx=ctx)
    s.SetRansacParameters(0.99, 8, MAX_ITS, 4, 0.4, 5.991)
    return s


def _same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, key)


def test_both_routes_store_the_same_bits_and_iterate_alike(ctx, world):
    a, f = _by_arrays(ctx, world), _by_frames(ctx, world)
    n_found = n_records = 0
    for k, n in enumerate(SIZES):
        ha, hf = a.hypotheses(k), f.hypotheses(k)
        assert len(ha["count"]) == a.state(k)["max_iterations"] + RESERVE > 0 and ha["inlier"].shape[1] == n
        _same(ha, hf, ("hypotheses", k))
        ra, rf = a.refinements(k), f.refinements(k)
        _same(ra, rf, ("refinements", k))
        n_records += len(ra["hyp"])
        assert a.state(k) == f.state(k)
        for turn in range(MAX_ITS // 5 + 2):                                # iterate(5) until the solver is done, as Relocalization does
            oa, of = a.iterate(k, 5), f.iterate(k, 5)
            assert (oa[0] is None) == (of[0] is None) and oa[1] == of[1] and oa[3] == of[3], (k, turn)
            assert oa[2].shape == (N_CUR,) and (oa[2] == of[2]).all()
            if oa[0] is not None:
                assert oa[0].tobytes() == of[0].tobytes()
                n_found += 1
            assert a.state(k) == f.state(k)
            if oa[1] or oa[0] is not None:
                break
    assert n_found >= 2 and n_records >= 2                                  # the poses were worth comparing
    a.close(); f.close()


def test_the_gathered_arrays_are_the_constructor_loop(ctx, world):
    """Independent of the array route: inlier flags and counts are exact functions of the reported double pose and of P2D, P3D and
    max_err (pnp_solver_ref.check_inliers), so they equal the restatement's only if every gathered value is the restated one."""
    Cq, S = world["Cq"], world["S"]
    f = _by_frames(ctx, world)
    rows = inl = 0
    for k in range(len(SIZES)):
        e = slice(Cq["first"][k], Cq["first"][k + 1])
        for tap in (f.hypotheses(k), f.refinements(k)):
            want = P.check_inliers(tap["Rt"], S["K"][k], Cq["P3Dw"][e], Cq["P2D"][e], P.max_error(Cq["sigma2"][e], 5.991))
            assert (tap["inlier"] == want).all() and (tap["count"] == want.sum(1)).all(), k
            rows += len(want); inl += int(want.sum())
    assert rows >= 100 and inl >= 300
    f.close()


def _create_raw(ctx, world, feature, slot, n_levels=N_LEVELS, sentinel=0x5A5A):
    Cq = world["Cq"]
    p = _lib.ptr
    feature = np.ascontiguousarray(feature, "i4"); slot = np.ascontiguousarray(slot, "i4")
    d = np.ascontiguousarray(world["draws"])
    fp = _lib.PnpFramesProblem(len(SIZES), p(Cq["first"]), p(world["S"]["K"]), p(feature), p(slot), p(SIGMA2), n_levels, 0.99, 8, MAX_ITS, 4, 0.4,
                               5.991, RESERVE, p(d), 0)
    h = C.c_void_p(sentinel)
    rc = ctx.lib.ccm_pnp_solver_create_frames(ctx.handle, C.c_void_p(world["cur"].handle), C.c_void_p(world["table"].handle), C.byref(fp), C.byref(h))
    return rc, h.value


def test_misuse_is_an_argument_error_and_leaves_out_alone(ctx, world):
    Cq = world["Cq"]
    e = int(Cq["first"][2]) + 3                                             # a correspondence of the last solver, past lane 64 of the launch
    cases = {}
    s = Cq["slot"].copy(); s[e] = 0; cases["a slot that is not LIVE"] = (Cq["feature"], s, N_LEVELS)
    s = Cq["slot"].copy(); s[e] = world["S"]["cap"]; cases["a slot outside the table"] = (Cq["feature"], s, N_LEVELS)
    s = Cq["slot"].copy(); s[e] = -1; cases["a negative slot"] = (Cq["feature"], s, N_LEVELS)
    f = Cq["feature"].copy(); f[e] = N_CUR; cases["feature N_cur"] = (f, Cq["slot"], N_LEVELS)
    top = int(world["S"]["oct"][Cq["feature"]].max())
    cases["an octave beyond the levels"] = (Cq["feature"], Cq["slot"], top)         # n_levels = the highest octave in use
    cases["no levels"] = (Cq["feature"], Cq["slot"], 0)
    for what, (feat, slot, nl) in cases.items():
        rc, h = _create_raw(ctx, world, feat, slot, nl)
        assert rc == E_ARG and h == 0x5A5A, what
        assert ctx.lib.ccm_last_error(ctx.handle) != b"", what
    rc, h = _create_raw(ctx, world, Cq["feature"], Cq["slot"])              # the context and the handles are fine afterwards
    assert rc == 0 and h not in (0, 0x5A5A, None)
    ctx.lib.ccm_pnp_solver_destroy(C.c_void_p(h))
    s = Cq["slot"].copy(); s[e] = 1                                         # BAD but LIVE is the caller's business: gathered like any other
    rc, h = _create_raw(ctx, world, Cq["feature"], s)
    assert rc == 0
    ctx.lib.ccm_pnp_solver_destroy(C.c_void_p(h))
