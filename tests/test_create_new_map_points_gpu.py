"""ccm_create_new_map_points (LocalMapping::CreateNewMapPoints, src/Mapping.cpp:284-469) on the GPU against the oracle's
SearchForTriangulation and the float64 restatement in tests/create_new_map_points_ref.py.

One module fixture calls the library once per case: the scene of ref.make_scene (3826 features in the current keyframe, 21 neighbours:
one the baseline rule skips, one of mostly low parallax, node ranges of 63, 64, 65 and 130 candidate features, exact duplicates on both
sides, a neighbour that stands beyond the near points) and the small cases of ref.SMALL_CASES (n_kf = 1, 2, 3; n1 = 1, 63, 64, 65; a
neighbour without features; a neighbour that shares no node with the current keyframe; every current feature already holding a map
point).  The oracle's matches and the float64 evaluation of the device's pairs are computed once, in the fixture.

Bound on the point: |X - X_ref|inf / depth <= 1.58e-5 = 4 x 3.94e-6, the worst value tools/create_new_map_points_study.py prints for
float32 storage in the operation order of csrc/map_math.h against float64 on these cases and this seed (20,856 matched pairs, 201 of
them ambiguous = 0.964 %, no status difference outside the bands).

The replay test states the specified rule (the rows of tap.match[k] whose status is neither SUPERSEDED nor HAS_MP) with one correction.  A feature that won with neighbour k' holds a map point for every later
neighbour, so the reference does not match it there at all.  The device's row for such a (k, i1) is SUPERSEDED only if its pair passes
every gate; a pair that fails a gate keeps that gate's code.  The rows compared with the replayed oracle are therefore those whose
status is neither SUPERSEDED nor HAS_MP and whose feature has not won before k."""
import ctypes as C

import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.mapping import LocalMapping, MapKeyFrame
from motioncheck_ccm_slam_amd.matcher import ORBmatcher
import create_new_map_points_ref as ref

pytestmark = pytest.mark.gpu

TOL_X = 1.58e-5
S = ref.S


def _kf(d):
    return MapKeyFrame(d["kp_x"], d["kp_y"], d["kp_octave"], d["desc"], d["node"], d["has_mp"], d["K"], d["Tcw"], d["Ow"],
                       d["scale_factors"], d["level_sigma2"])


def _search_args(sc, k, has_mp1):
    cur, kf = sc["current"], sc["neighbours"][k]
    ex, ey = sc["epipole"][k]
    return (cur["desc"], cur["node"], has_mp1, cur["kp_x"], cur["kp_y"], np.zeros(len(cur["kp_x"]), "f4"), kf["desc"], kf["node"], kf["has_mp"],
            kf["kp_x"], kf["kp_y"], np.zeros(len(kf["kp_x"]), "f4"), kf["kp_octave"], sc["F12"][k], float(ex), float(ey), kf["scale_factors"],
            kf["level_sigma2"])


def _call(ctx, sc, tap=True):
    lm = LocalMapping(ctx=ctx)
    n_new, kf, idx1, idx2, x3d, first = lm.CreateNewMapPoints(_kf(sc["current"]), [_kf(k) for k in sc["neighbours"]], sc["median_depth"],
                                                              F12=sc["F12"], epipole=sc["epipole"], tap=tap)
    out = dict(n_new=n_new, kf=kf.copy(), idx1=idx1.copy(), idx2=idx2.copy(), x3d=x3d.copy(), first=first.copy())
    if tap:
        out.update({k: v.copy() for k, v in lm.tap().items()})
    return out


def run_all(ctx, oracle):
    scene = ref.make_scene()
    cases = [scene] + [ref.make_small(scene, n1, ks, **kw) for n1, ks, kw in ref.SMALL_CASES]
    runs = []
    for sc in cases:
        cur = sc["current"]
        sc["epipole"] = np.array([ref.epipole32(cur, kf) for kf in sc["neighbours"]], "f4").reshape(-1, 2)
        r = _call(ctx, sc)
        r["sc"] = sc
        r["skipped"] = [ref.baseline_too_short(cur["Ow"], kf["Ow"], md) for kf, md in zip(sc["neighbours"], sc["median_depth"])]
        r["oracle"] = [oracle.search_for_triangulation(*_search_args(sc, k, cur["has_mp"]), 0)[1] for k in range(len(sc["neighbours"]))]
        r["f64"] = []                                                          # the float64 evaluation of the device's own pairs
        for k, kf in enumerate(sc["neighbours"]):
            i1 = np.flatnonzero(r["match"][k] >= 0)
            r["f64"].append((i1, r["match"][k][i1], ref.pairs_ref(cur, kf, i1, r["match"][k][i1])))
        runs.append(r)
    return runs


@pytest.fixture(scope="module")
def runs(ctx, oracle):
    return run_all(ctx, oracle)


def _gate(status):
    """the status before the resolution: SUPERSEDED rows passed every gate"""
    return np.where(status == S["SUPERSEDED"], S["OK"], status)


def test_match_half_is_exact(ctx, oracle, runs):
    """tap.match equals the oracle's SearchForTriangulation (no orientation filter) and ccm_search_for_triangulation on the flags as
    they stood on entry, bit for bit, for every neighbour; and the reference's loop, replayed with the device's own winners flagged
    before each neighbour, matches exactly the rows the device left live (module docstring): the separability argument."""
    m = ORBmatcher(0.6, False, ctx=ctx)
    r = runs[0]
    sc = r["sc"]; cur = sc["current"]
    busy = shared = ties = dead_rows = 0
    for r in runs:
        sc = r["sc"]; cur = sc["current"]
        n_kf = len(sc["neighbours"])
        for k in range(n_kf):
            assert (r["match"][k] == r["oracle"][k]).all(), k
            assert (r["match"][k][cur["has_mp"] != 0] == -1).all()
        for k in (range(n_kf) if r is runs[0] else range(min(n_kf, 1))):       # the old single-pair entry point: every neighbour of the scene
            assert (m.SearchForTriangulation(*_search_args(sc, k, cur["has_mp"]))[1] == r["match"][k]).all(), k
        has_mp1 = cur["has_mp"].copy()
        for k in range(n_kf):
            replay = oracle.search_for_triangulation(*_search_args(sc, k, has_mp1), 0)[1]
            won_before = (has_mp1 != 0) & (cur["has_mp"] == 0)
            st = r["status"][k]
            live = (st != S["SUPERSEDED"]) & (st != S["HAS_MP"]) & ~won_before
            assert (replay == np.where(live, r["match"][k], -1)).all(), k
            dead_rows += int((won_before & (r["match"][k] >= 0) & (st != S["SUPERSEDED"])).sum())
            has_mp1[r["idx1"][r["kf"] == k]] = 1
    r = runs[0]
    for k, kf in enumerate(r["sc"]["neighbours"]):
        mk = r["match"][k][r["match"][k] >= 0]
        busy += int(len(mk) >= 100)
        shared += int((np.bincount(mk, minlength=1) >= 2).sum())
        ties += int((kf["copy_of"][mk] >= 0).sum())
        originals = kf["copy_of"][kf["copy_of"] >= 0]
        assert not np.isin(mk, originals).any(), k                            # equal distance: the last in node order wins
    print("neighbours with >= 100 matches: %d, idx2 chosen twice: %d, ties: %d, matched rows of features that had won: %d" % (busy, shared, ties, dead_rows))
    assert busy >= 15 and shared >= 10 and ties >= 10 and dead_rows >= 10


def test_gates_follow_the_devices_own_point_exactly(runs):
    """ref.gates32, a float32 numpy evaluation of :399-448 in the operation order of csrc/map_math.h, fed with the device's x3d_all
    reproduces every status from the depth test onwards; rows without a point hold zeros."""
    checked = 0
    for r in runs:
        sc = r["sc"]
        for k, kf in enumerate(sc["neighbours"]):
            st = _gate(r["status"][k])
            rows = np.flatnonzero(st >= S["BEHIND_1"])
            assert (r["match"][k][rows] >= 0).all()
            assert (ref.gates32(sc["current"], kf, rows, r["match"][k][rows], r["x3d_all"][k][rows]) == st[rows]).all(), k
            assert (r["x3d_all"][k][st < S["NONFINITE"]] == 0).all() and np.isfinite(r["x3d_all"][k]).all()
            checked += len(rows)
    assert checked >= 15000


def test_statuses_and_points_against_float64(runs):
    """Outside ambiguous pairs every status equals the float64 restatement's; points of pairs that pass every gate in both are within
    the bound (module docstring).  Cap, a condition on the scene: ambiguous <= 1 % of the matched pairs.  Coverage of the scene."""
    pairs = amb_n = 0; worst = 0.0
    for r in runs:
        for k, (i1, i2, w) in enumerate(r["f64"]):
            st = r["status"][k]
            if r["skipped"][k]:
                assert (st == S["SKIPPED_KF"]).all() and (r["x3d_all"][k] == 0).all(), k
                continue
            assert (st != S["SKIPPED_KF"]).all()
            assert ((st == S["HAS_MP"]) == (r["sc"]["current"]["has_mp"] != 0)).all()
            assert ((st == S["NO_MATCH"]) == ((r["match"][k] < 0) & (r["sc"]["current"]["has_mp"] == 0))).all()
            g = _gate(st[i1])
            wrong = (g != w["status"]) & ~w["ambiguous"]
            assert not wrong.any(), (k, i1[wrong][:5], g[wrong][:5], w["status"][wrong][:5])
            both = (g == S["OK"]) & (w["status"] == S["OK"])
            if both.any():
                dx = np.abs(r["x3d_all"][k][i1[both]].astype("f8") - w["X"][both]).max(1) / np.abs(w["z1"][both])
                worst = max(worst, float(dx.max()))
                assert dx.max() <= TOL_X, (k, float(dx.max()))
            pairs += len(i1); amb_n += int(w["ambiguous"].sum())
    r = runs[0]
    count = np.bincount(r["status"].ravel(), minlength=len(ref.STATUS))
    matched = int(sum(len(i1) for (i1, _, _), sk in zip(r["f64"], r["skipped"]) if not sk))
    print("matched pairs %d (scene %d), ambiguous %d (%.3f %%), worst |dX|/depth %.3g (bound %.3g)" % (pairs, matched, amb_n, 100.0 * amb_n / pairs, worst, TOL_X))
    print({ref.STATUS[s]: int(count[s]) for s in np.flatnonzero(count)})
    assert amb_n <= 0.01 * pairs
    assert matched >= 3000
    assert count[S["OK"]] >= 1000 and count[S["LOW_PARALLAX"]] >= 100 and count[S["BEHIND_1"]] >= 20
    assert count[S["REPROJ_1"]] + count[S["REPROJ_2"]] >= 50 and count[S["SCALE"]] >= 50 and count[S["BEHIND_2"]] >= 1
    assert count[S["SUPERSEDED"]] >= 50
    assert r["skipped"] == [True] + [False] * 20 and (r["status"][0] == S["SKIPPED_KF"]).all()


def test_list_is_the_references(ctx, oracle, runs):
    """kf / idx1 / idx2 / x3d / first equal what the reference's loop creates when it runs on the oracle's SearchForTriangulation with
    the flags updated as it goes and on the device's own gate results; a call without a tap returns the same bytes."""
    for c, r in enumerate(runs):
        sc = r["sc"]; cur = sc["current"]
        n_kf = len(sc["neighbours"])

        def search(k, has_mp1):
            return oracle.search_for_triangulation(*_search_args(sc, k, has_mp1), 0)[1]

        def pair_status(k, i1, i2):
            assert (r["match"][k][i1] == i2).all()
            return _gate(r["status"][k][i1]), r["x3d_all"][k][i1]

        rows, first = ref.create_new_map_points(sc, search, pair_status)
        assert r["n_new"] == len(rows) == r["first"][n_kf] and (r["first"] == first).all(), c
        assert r["kf"].tolist() == [x[0] for x in rows] and r["idx1"].tolist() == [x[1] for x in rows] and r["idx2"].tolist() == [x[2] for x in rows]
        assert r["x3d"].tobytes() == np.array([x[3] for x in rows], "f4").reshape(-1, 3).tobytes()
        assert len(set(r["idx1"].tolist())) == r["n_new"] and (np.diff(r["first"]) >= 0).all() and r["first"][0] == 0
        assert (cur["has_mp"][r["idx1"]] == 0).all()
        for k in range(n_kf):                                                  # the rows of neighbour k: its OK rows, idx1 ascending
            seg = slice(r["first"][k], r["first"][k + 1])
            assert (r["kf"][seg] == k).all() and (r["idx1"][seg] == np.flatnonzero(r["status"][k] == S["OK"])).all()
        plain = _call(ctx, sc, tap=False)
        for key in ("kf", "idx1", "idx2", "x3d", "first"):
            assert plain[key].tobytes() == r[key].tobytes(), (c, key)
        assert plain["n_new"] == r["n_new"]
    assert runs[0]["n_new"] >= 1000
    by_n1 = {len(r["sc"]["current"]["kp_x"]): r["n_new"] for r in runs[1:5]}
    assert set(by_n1) == {1, 63, 64, 65} and all(v > 0 for k, v in by_n1.items() if k > 1)
    assert runs[-1]["n_new"] == 0 and (runs[-1]["status"] == S["HAS_MP"]).all()                    # every feature flagged
    foreign = runs[-2]
    assert (foreign["status"][0] == S["NO_MATCH"]).all() and foreign["first"][1] == 0 and foreign["n_new"] > 0
    empty = runs[-3]
    assert (empty["status"][1] == S["NO_MATCH"]).all() and empty["first"][1] == empty["first"][2] and empty["n_new"] > 0


def test_second_call_returns_identical_bytes(ctx, runs):
    for r in (runs[0], runs[3], runs[5]):
        again = _call(ctx, r["sc"])
        assert again["n_new"] == r["n_new"]
        for key in ("kf", "idx1", "idx2", "x3d", "first", "match", "status", "x3d_all"):
            assert again[key].tobytes() == r[key].tobytes(), key


def test_hundred_calls_reuse_the_context_pool(ctx, runs):
    import torch
    free10 = None
    for i in range(100):
        r = runs[(0, 3, 2)[i % 3]]
        assert _call(ctx, r["sc"], tap=False)["n_new"] == r["n_new"]
        if i == 9:
            free10 = torch.cuda.mem_get_info()[0]
    assert torch.cuda.mem_get_info()[0] == free10


def test_argument_errors_name_the_argument_and_leave_the_outputs_untouched(ctx, runs):
    sc = runs[3]["sc"]                                                         # 64 features, three neighbours
    cur = _kf(sc["current"]); nbs = [_kf(k) for k in sc["neighbours"]]
    lib = ctx.lib; q = _lib.ptr
    n1, n_kf = cur.n, len(nbs)

    def call(over, n_kf=n_kf, drop=(), cur=cur, nbs=nbs):
        a = dict(F12=sc["F12"], epipole=sc["epipole"], median_depth=sc["median_depth"])
        a.update(over)
        cs = cur.as_struct()
        arr = (_lib.MapKeyframe * len(nbs))(*[k if isinstance(k, _lib.MapKeyframe) else k.as_struct() for k in nbs])
        pb = _lib.NewPointsProblem(C.pointer(cs), n_kf, arr, q(a["F12"]), q(a["epipole"]), q(a["median_depth"]))
        o = dict(kf=np.full(n1, 7, "i4"), idx1=np.full(n1, 7, "i4"), idx2=np.full(n1, 7, "i4"), x3d=np.full((n1, 3), 7.0, "f4"),
                 first=np.full(len(nbs) + 1, 7, "i4"), match=np.full(len(nbs) * n1, 7, "i4"), status=np.full(len(nbs) * n1, 77, "u1"),
                 x3d_all=np.full((len(nbs) * n1, 3), 7.0, "f4"))
        for key in drop:
            o[key] = None
        tp = _lib.NewPointsTap(q(o["match"]), q(o["status"]), q(o["x3d_all"]))
        res = _lib.NewPointsResult(77, q(o["kf"]), q(o["idx1"]), q(o["idx2"]), q(o["x3d"]), q(o["first"]), C.pointer(tp))
        rc = lib.ccm_create_new_map_points(ctx.handle, C.byref(pb), C.byref(res))
        clean = res.n_new == 77 and all(v is None or (v == (77 if key == "status" else 7)).all() for key, v in o.items())
        return rc, lib.ccm_last_error(ctx.handle).decode(), clean

    bad_oct = _kf(sc["neighbours"][2]); bad_oct.kp_octave = bad_oct.kp_octave.copy(); bad_oct.kp_octave[5] = 8
    neg_oct = _kf(sc["current"]); neg_oct.kp_octave = neg_oct.kp_octave.copy(); neg_oct.kp_octave[63] = -1
    big_node = _kf(sc["neighbours"][0]); big_node.node = big_node.node.copy(); big_node.node[0] = 1 << 24
    no_x = nbs[1].as_struct(); no_x.kp_x = None
    no_tcw = cur.as_struct(); no_tcw.Tcw = None
    md = sc["median_depth"]
    for kw, word in ((dict(n_kf=-1), "n_kf"), (dict(over=dict(F12=None)), "F12"), (dict(over=dict(epipole=None)), "epipole"),
                     (dict(over=dict(median_depth=None)), "median_depth"),
                     (dict(over=dict(median_depth=np.array([md[0], 0.0, md[2]], "f4"))), "median_depth[1]"),
                     (dict(over=dict(median_depth=np.array([md[0], md[1], np.nan], "f4"))), "median_depth[2]"),
                     (dict(nbs=[nbs[0], nbs[1], bad_oct]), "neighbours[2].kp_octave[5]"), (dict(cur=neg_oct), "current.kp_octave[63]"),
                     (dict(nbs=[big_node, nbs[1], nbs[2]]), "neighbours[0].node[0]"), (dict(nbs=[nbs[0], no_x, nbs[2]]), "neighbours[1].kp_x"),
                     (dict(drop=("first",)), "first"), (dict(drop=("x3d",)), "x3d"), (dict(drop=("kf",)), "kf")):
        rc, err, clean = call(kw.pop("over", {}), **kw)
        assert rc == -1 and word in err and clean, (word, rc, err, clean)
    cs_arr = (_lib.MapKeyframe * n_kf)(*[k.as_struct() for k in nbs])
    pb = _lib.NewPointsProblem(C.pointer(no_tcw), n_kf, cs_arr, q(sc["F12"]), q(sc["epipole"]), q(md))
    res = _lib.NewPointsResult(77, None, None, None, None, None, None)
    assert lib.ccm_create_new_map_points(ctx.handle, C.byref(pb), C.byref(res)) == -1 and "current.Tcw" in lib.ccm_last_error(ctx.handle).decode()
    assert lib.ccm_create_new_map_points(ctx.handle, None, C.byref(res)) == -1 and "problem" in lib.ccm_last_error(ctx.handle).decode()
    assert lib.ccm_create_new_map_points(ctx.handle, C.byref(pb), None) == -1 and "result" in lib.ccm_last_error(ctx.handle).decode()
    assert res.n_new == 77
    # empty inputs are valid: 0 new points
    lm = LocalMapping(ctx=ctx)
    out = lm.CreateNewMapPoints(cur, [], [])
    assert out[0] == 0 and out[5].tolist() == [0]
    none = _kf(ref.subset(sc["current"], np.arange(0)))
    out = lm.CreateNewMapPoints(none, nbs, md, F12=sc["F12"], epipole=sc["epipole"])
    assert out[0] == 0 and out[5].tolist() == [0, 0, 0, 0] and lm.tap()["status"].shape == (3, 0)
    out = lm.CreateNewMapPoints(cur, [_kf(ref.subset(k, np.arange(0))) for k in sc["neighbours"]], md, F12=sc["F12"], epipole=sc["epipole"])
    assert out[0] == 0 and (lm.tap()["status"] == S["NO_MATCH"]).all()
