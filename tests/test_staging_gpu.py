"""The per-call staging block (csrc/staging.h) re-used or re-allocated while an asynchronous upload from it is still queued.

An upload leaves the page-locked host block busy until the copy has run; the next call that fills the block has to wait for it, and
a call that needs a larger block frees and re-allocates it right behind the queued copy.  Nothing else in the suite issues such
calls back to back without a synchronisation in between.  Every test starts on a fresh Context, whose blocks are at their smallest;
everything compared is byte for byte (what was sent, or the same problem on another fresh context)."""
import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.initializer import Initializer
from motioncheck_ccm_slam_amd.mapping import LocalMapping, MapKeyFrame
from motioncheck_ccm_slam_amd.matcher import FrameGridView
from motioncheck_ccm_slam_amd.sim3solver import Sim3Solver, make_draws
from motioncheck_ccm_slam_amd.tracking import MapPointTable
import create_new_map_points_ref as map_ref
import initializer_ref as ini_ref
import keyframe_handles_ref as kf_ref
import sim3_solver_ref as sim3_ref
from test_frame_gpu import _np_grid

pytestmark = pytest.mark.gpu

COLS = ("pos", "normal", "min_dist", "max_dist", "desc", "flags")
CAPACITY = 8192


@pytest.fixture
def fresh(ctx):
    """A factory of new contexts (behind the session's one, which settles which HIP runtime the process uses), closed at the end."""
    made = []

    def make():
        made.append(_lib.Context(0))
        return made[-1]
    yield make
    for c in made:
        c.close()


def _rows(rng, slots):
    n = len(slots)
    return dict(slot=np.asarray(slots, "i4"), pos=rng.normal(0, 5, (n, 3)).astype("f4"), normal=rng.normal(0, 1, (n, 3)).astype("f4"),
                min_dist=rng.uniform(0.1, 1, n).astype("f4"), max_dist=rng.uniform(5, 50, n).astype("f4"),
                desc=rng.integers(0, 256, (n, 32)).astype(np.uint8), flags=rng.integers(1, 4, n).astype(np.uint8))


def _update(table, rows):
    table.update(rows["slot"], *[rows[k] for k in COLS])


def _check_table(table, updates):
    """Every touched slot holds the row of the last update that names it."""
    want = {}
    for rows in updates:
        for r, s in enumerate(rows["slot"].tolist()):
            want[s] = (rows, r)
    slots = np.array(sorted(want), "i4")
    got = table.fetch(slots)
    for k in COLS:
        sent = np.stack([want[s][0][k][want[s][1]] for s in slots.tolist()])
        assert got[k].tobytes() == sent.tobytes(), k


@pytest.mark.parametrize("sizes", [(1, 5000), (5000, 1, 5000)], ids=["grow-behind-a-queued-copy", "reuse-only"])
def test_table_updates_back_to_back(fresh, sizes):
    rng = np.random.default_rng(7)
    free = rng.permutation(CAPACITY)
    updates = []
    with MapPointTable(CAPACITY, ctx=fresh()) as t:
        for n in sizes:                                                    # no synchronisation in between
            # the single row has a slot of its own; every 5,000-row update draws from the others (two of them share about 3,000 slots)
            updates.append(_rows(rng, free[:1] if n == 1 else rng.choice(free[1:], n, replace=False)))
            assert len(updates[-1]["slot"]) == n
            _update(t, updates[-1])
        big = next(u for u in updates if len(u["slot"]) == 5000)
        updates.append(_rows(rng, rng.choice(big["slot"], 64, replace=False)))      # 64 rows over some of the first 5,000
        _update(t, updates[-1])
        _check_table(t, updates)


def _view(rng, n):
    return FrameGridView(rng.uniform(0, 752, n), rng.uniform(0, 480, n), rng.integers(0, 8, n), rng.integers(0, 256, (n, 32)))


def test_frame_setters_back_to_back(fresh):
    rng = np.random.default_rng(8)
    c = fresh()
    sf = (1.2 ** np.arange(8)).astype("f4")
    v_small, v_large = _view(rng, 1), _view(rng, 2049)
    # the two creations are where the block grows behind a queued copy (4 KB, then about 98 KB); every later call re-uses it
    with DeviceFrame(v_small, ctx=c) as small, DeviceFrame(v_large, ctx=c) as large, MapPointTable(CAPACITY, ctx=c) as t:
        ids_small = np.array([4711], "i4"); ids_large = rng.integers(-1, CAPACITY, 2049).astype("i4")
        small.map_points = ids_small                                       # small, then large, back to back
        large.map_points = ids_large
        node = rng.integers(-1, 40, 2049).astype("i4")
        T = np.eye(3, 4, dtype="f4"); T[:, 3] = (0.1, 0.2, 0.3)
        rows_a, rows_b = _rows(rng, np.arange(100, 700)), _rows(rng, np.arange(400, 403))
        large.set_pose(T, -T[:, 3])
        _update(t, rows_a)
        large.set_camera((458.0, 457.0, 367.0, 248.0), sf, sf * sf)
        large.set_bow(node)
        _update(t, rows_b)
        large.set_pose(T, -T[:, 3])
        assert small.map_points.tobytes() == ids_small.tobytes()
        assert large.map_points.tobytes() == ids_large.tobytes()
        for got, want in zip(large.bow(), kf_ref.directory(node)):
            assert got.tobytes() == want.tobytes()
        for h, v in ((small, v_small), (large, v_large)):                  # the grid is built from the coordinates each creation uploaded
            for got, want in zip(h.grid(), _np_grid(v)):
                assert got.tobytes() == want.tobytes()
        _check_table(t, [rows_a, rows_b])


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _same(a[k], b[k], "%s.%s" % (path, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), path
    else:
        assert a == b, path


def _small_then_large(fresh, run, small, large):
    """run(ctx, problem) on one fresh context for the small and then the large problem, and for the large one alone on another."""
    c = fresh()
    run(c, small)
    got = run(c, large)
    _same(got, run(fresh(), large))
    return got


def test_initializer_small_then_large(fresh):
    rng = np.random.default_rng(9)

    def problem(n, its):
        p = ini_ref.make_two_view(rng, n, 0.2 if n > 8 else 0.0, "general")
        return p, rng.integers(0, np.broadcast_to(np.maximum(n - np.arange(8), 1), (its, 8))).astype("i4")

    def run(c, pd):
        p, d = pd
        ini = Initializer(p["kp1"], p["K"], p["sigma"], len(d), ctx=c)
        out = ini.Initialize(p["kp2"], p["matches12"], d)
        return dict(out=out, res=ini.result, hyp=ini.hypotheses(), cand=ini.candidates())
    got = _small_then_large(fresh, run, problem(8, 8), problem(800, 200))
    assert got["res"]["n_matches"] == 800 and got["res"]["best_f"] >= 0


def _kf(d):
    return MapKeyFrame(d["kp_x"], d["kp_y"], d["kp_octave"], d["desc"], d["node"], d["has_mp"], d["K"], d["Tcw"], d["Ow"],
                       d["scale_factors"], d["level_sigma2"])


def test_create_new_map_points_small_then_large(fresh):
    scene = map_ref.make_scene()                                           # 3826 features, 21 neighbours
    n1, ks, kw = map_ref.SMALL_CASES[0]                                    # one feature, one neighbour
    cases = [map_ref.make_small(scene, n1, ks, **kw), scene]
    for sc in cases:
        sc["epipole"] = np.array([map_ref.epipole32(sc["current"], kf) for kf in sc["neighbours"]], "f4").reshape(-1, 2)

    def run(c, sc):
        lm = LocalMapping(ctx=c)
        n_new, kf, idx1, idx2, x3d, first = lm.CreateNewMapPoints(_kf(sc["current"]), [_kf(k) for k in sc["neighbours"]], sc["median_depth"],
                                                                  F12=sc["F12"], epipole=sc["epipole"], tap=True)
        return dict(n_new=n_new, kf=kf.copy(), idx1=idx1.copy(), idx2=idx2.copy(), x3d=x3d.copy(), first=first.copy(),
                    tap={k: v.copy() for k, v in lm.tap().items()})
    got = _small_then_large(fresh, run, *cases)
    assert got["n_new"] > 100


def test_sim3_solver_small_then_large(fresh):
    rng = np.random.default_rng(10)

    def problem(n, share, min_inliers, its):
        p = sim3_ref.make_solver_problem(rng, n, share, False)
        return [p], make_draws(rng, [n], its), min_inliers, its

    def run(c, pb):
        problems, draws, min_inliers, its = pb
        s = Sim3Solver(draws=draws, ctx=c, **sim3_ref.flatten(problems))
        s.SetRansacParameters(0.99, min_inliers, its)
        out = dict(hyp=s.hypotheses(0), find=s.find(0), state=s.state(0))
        s.close()
        return out
    got = _small_then_large(fresh, run, problem(3, 0.0, 3, 300), problem(300, 0.5, 6, 300))
    assert len(got["hyp"]["count"]) == 300
