"""tests/window_matcher_ref.py (the windowed matchers restated from the reference's text) held to three things, without a GPU:
answers written down by hand for every hand-built case of tests/window_matcher_cases.py, with the decisions a case is built to
force asserted from the definition's own trace; bit equality with the CPU oracle, on the hand-built cases and on the random scenes
of test_window_gpu.py (fed from the oracle's own extraction); and seven deliberately wrong variants of the definition, each of
which must change the output of at least one hand-built case."""
import numpy as np
import pytest

import window_matcher_cases as C
import window_matcher_ref as R
from motioncheck_ccm_slam_amd import synth


def norm(o):
    """Nested lists of Python numbers, so that == compares everything."""
    if isinstance(o, (list, tuple)):
        return [norm(x) for x in o]
    if isinstance(o, np.ndarray):
        return o.tolist()
    return o.item() if isinstance(o, np.generic) else o


# Derived by hand from the reference's text, case by case (the derivations are the builders' docstrings):
# area: one index list per query; projection / frame: (nmatches, match per feature, occupied); sim3: (nmatches, best_idx per point,
# matched); fuse: (best_idx, best_dist); by_sim3: (nFound, match12); init: (nmatches, matches12, prev_matched).
HAND = {
    "area_radius_edge": [[5, 3, 1]],
    "area_zero_outside_whole": [[], [], [], [], [], [3, 2, 1, 4, 0]],
    "area_max_x": [[1]],
    "area_half_cells": [[1, 0], [3], [4]],
    "area_levels": [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0], [1, 2, 3, 4], [2, 3]],
    "proj_tie_order": [1, [-1, 0], [0, 1]],
    "sim3_tie_order": [1, [1], [0, 1]],
    "frame_tie_order": [1, [-1, 0], [0, 1]],
    "fuse_tie_order": [[1], [20]],
    "proj_thresholds": [3, [0, -1, 2, -1, -1, -1, 4, -1], [1, 0, 1, 0, 0, 0, 1, 0]],
    "sim3_thresholds": [2, [0, -1, 3], [1, 0, 0, 1]],
    "frame_thresholds_64": [2, [0, -1, -1, 2], [1, 0, 0, 1]],
    "frame_thresholds_100": [2, [0, -1, -1, 2], [1, 0, 0, 1]],
    "fuse_thresholds_50": [[0, -1, 3, -1], [50, 51, 30, 256]],
    "fuse_thresholds_100": [[0, -1, 3, -1], [100, 101, 30, 256]],
    "fuse_chi2": [[0, 2], [10, 30]],
    "proj_order_a": [5, [4], [0]],
    "proj_order_b": [3, [0, 1, 2], [1, 1, 1]],
    "proj_order_cd": [3, [1, 0, 3, -1], [1, 1, 1, 0]],
    "sim3_order_e": [2, [0, 0, 1, 1, -1], [1, 1]],
    "frame_hist_ties": [8, [-1, 1, 2, 3, 4, 5, 6, 7, -1, -1], [1] * 10],
    "frame_hist_tenth_10": [11, list(range(11)), [1] * 11],
    "frame_hist_tenth_11": [11, list(range(11)) + [-1], [1] * 12],
    "by_sim3_agreement": [1, [0, -1, -1]],
    "init_basic": [3, [-1, 0, -1, 1, 2, -1, -1], [[100, 100], [100, 100], [100, 100], [103, 100], [300, 100], [400, 100], [501, 100]]],
}


def closed_form(case):
    """The answer of a kernel-size case from its construction (window_matcher_cases.size_chain / size_sparse / cand_counts /
    cand_positions)."""
    name, kind = case["name"], case["kind"]
    n_feat = len(case["grid"]["kx"])
    n_pts = len(case["args"]["u" if kind != "projection" else "proj_x"])
    per_feature = np.full(n_feat, -1, np.int64); per_point = np.full(n_pts, -1, np.int64)
    if name.startswith("size_chain"):                               # point m takes feature m (distance m + 1) up to the threshold
        for m in range(min(n_pts, 50 if kind == "sim3" else 100)):
            per_feature[m] = m; per_point[m] = m
    elif name.startswith("size_sparse"):                            # point j * stride sits on feature j
        stride = max(1, n_pts // 200)
        for j in range(200):
            if j * stride < n_pts:
                per_feature[j] = j * stride; per_point[j * stride] = j
    elif name.startswith("pos_"):                                   # cluster k (p + 2 features): its points take list positions p, p + 1, 0
        f0 = 0
        for k, p in enumerate(int(s) for s in name.split("_")[2:]):
            for q in range(3):
                j = f0 + (p if kind == "fuse" else (p + q) % (p + 2))
                per_feature[j] = 3 * k + q; per_point[3 * k + q] = j
            f0 += p + 2
    else:                                                           # clusters: the three points of a cluster take the features at distance 1, 2, 3
        sizes = [int(s) for s in name.split("_")[2:]]               # (fuse: each takes the one at distance 1)
        f0 = 0
        for k, c in enumerate(sizes):
            for p in range(3):
                want = 0 if kind == "fuse" else p
                j = [j for j in range(c) if (j * 37) % c == want]
                if j:
                    per_feature[f0 + j[0]] = 3 * k + p; per_point[3 * k + p] = f0 + j[0]
            f0 += c
    taken = (per_feature >= 0).astype(int).tolist()
    n = int((per_point >= 0).sum())
    if kind == "sim3":
        return [n, per_point.tolist(), taken]
    if kind == "fuse":
        dist = [1 if i >= 0 else 256 for i in per_point]
        return [per_point.tolist(), dist]
    return [n, per_feature.tolist(), taken]


BATCH_HAND = {
    # keyframe 0: feature 0 is matched on entry; keyframe 1: clusters of 65 and 17, points take distances 1, 2, 3 (feature j has distance
    # 1 + 37 j mod c: 0, 58, 51 of the 65; 65 + 0, 65 + 6, 65 + 12 of the 17); keyframe 2: no features; keyframe 3: no queries
    "batch_sim3": [[3, [1, -1, 2, 3, -1], [1, 1, 1, 1]],
                   [6, [0, 58, 51, 65, 71, 77], [1 if j in (0, 58, 51, 65, 71, 77) else 0 for j in range(82)]],
                   [0, [-1] * 25, []], [0, [], [0, 0]]],
    "batch_fuse": [[[0, 0, 2, 3, -1], [10, 10, 15, 50, 256]], [[0, 0, 0, 65, 65, 65], [1] * 6], [[-1] * 25, [256] * 25], [[], []]],
}


def run_oracle(O, case):
    k, a = case["kind"], case.get("args")
    if k.endswith("_batch"):
        return [run_oracle(O, s) for s in case["subs"]]
    if k == "by_sim3":
        g1, g2 = R.Grid(**case["grid1"]), R.Grid(**case["grid2"])
        return O.search_by_sim3(g1, a["sf1"], g2, a["sf2"], a["valid1"], a["u1"], a["v1"], a["level1"], a["mp_desc1"], a["valid2"], a["u2"], a["v2"],
                                a["level2"], a["mp_desc2"], a["th"])
    g = R.Grid(**case["grid"])
    gp = (g.kx, g.ky, g.oct, g.desc, g.min_x, g.min_y, g.inv_w, g.inv_h)
    if k == "area":
        return [O.features_in_area(g.kx, g.ky, g.oct, g.min_x, g.min_y, g.inv_w, g.inv_h, *q).tolist() for q in a["queries"]]
    if k == "init":
        return O.search_for_initialization(a["oct1"], a["desc1"], a["angle1"], g.kx, g.ky, g.oct, g.desc, g.angle, g.min_x, g.min_y, g.inv_w, g.inv_h,
                                           a["prev_matched"], a["window"], a["nnratio"], a["check_ori"])
    if k == "projection":
        return O.search_by_projection(*gp, a["scale_factors"], a["in_view"], a["level"], a["view_cos"], a["proj_x"], a["proj_y"], a["mp_desc"],
                                      a["has_obs"], a["occupied"], a["th"], a["nnratio"])
    if k == "frame":
        return O.search_by_projection_frame(*gp[:4], g.angle, *gp[4:], a["scale_factors"], a["valid"], a["u"], a["v"], a["last_octave"], a["last_angle"],
                                            a["mp_desc"], a["has_obs"], a["occupied"], a["th"], a["check_ori"], orb_dist=a["orb_dist"])
    if len(a["valid"]) == 0 or g.n == 0:                            # nothing to ask the oracle: the definition's empty answer stands
        return C.run_ref(case)
    if k == "sim3":
        return O.search_by_projection_sim3(g, a["scale_factors"], a["valid"], a["u"], a["v"], a["level"], a["mp_desc"], a["observed"], a["matched"], a["th"])
    return O.fuse_select(*gp, a["scale_factors"], a["inv_level_sigma2"], a["valid"], a["u"], a["v"], a["level"], a["mp_desc"], a["th"], a["chi2_check"],
                         accept_th=a["accept_th"])


@pytest.fixture(scope="module")
def ref_runs():
    """Every hand-built case through the definition once: name -> (case, output, trace)."""
    runs = {}
    for c in C.all_cases() + [C.batch("sim3"), C.batch("fuse")]:
        trace = {}
        runs[c["name"]] = (c, norm(C.run_ref(c, trace=trace)), trace)
    assert len(runs) == len(C.all_cases()) + 2                      # names are unique
    return runs


def _forced(case, trace):
    for key, least in case["forces"].items():
        assert trace.get(key, 0) >= least, (case["name"], key, trace)
    return ", ".join("%s=%d" % (k, trace[k]) for k in sorted(trace) if k in case["forces"]) or "-"


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_derived_answer(ref_runs, name):
    case, out, trace = ref_runs[name]
    assert out == HAND[name]
    print("%-26s forced: %s" % (name, _forced(case, trace)))


def test_every_small_case_has_a_hand_answer():
    assert sorted(c["name"] for c in C.small_cases()) == sorted(HAND)


def test_size_cases_follow_their_construction(ref_runs):
    for c in C.size_cases():
        case, out, trace = ref_runs[c["name"]]
        assert out == closed_form(case), c["name"]
        print("%-40s forced: %s" % (c["name"], _forced(case, trace)))
    forced = [ref_runs[c["name"]][2] for c in C.size_cases()]
    assert max(t["max_candidates"] for t in forced) == C.N_CHAIN    # the retry-sized lists exist (cap = 64 at first)
    assert {t["max_candidates"] for t in forced} >= {1, 64, 65, 200}  # the longest list of a case: below, at and past the first capacity
    assert max(t.get("candidate_taken_earlier", 0) for t in forced) == 2048


@pytest.mark.parametrize("kind", ["sim3", "fuse"])
def test_batch_cases_by_hand(ref_runs, kind):
    case, out, trace = ref_runs["batch_" + kind]
    assert out == BATCH_HAND["batch_" + kind]
    assert trace["max_candidates"] == 65                            # keyframe 1 forces the retry of every keyframe
    if kind == "sim3":
        assert case["subs"][0]["args"]["matched"].sum() == 1 and len(case["subs"][2]["grid"]["kx"]) == 0 and len(case["subs"][3]["args"]["u"]) == 0


def test_hand_built_cases_equal_the_oracle(oracle, ref_runs):
    for name, (case, out, _) in ref_runs.items():
        assert norm(run_oracle(oracle, case)) == out, name


# ------------------------------------------------------------------ the random scenes of test_window_gpu.py, extraction by the oracle
def _extract(O, f, nfeatures=1000, img=None):
    par = O.default_params(nfeatures, 1.2, 8, 20, 7)
    r = O.orb_extract(par, synth.frame(f) if img is None else img)
    k = r["kps"]
    return dict(kx=k["x"], ky=k["y"], octave=k["octave"], desc=r["desc"], angle=k["angle"]), O.orb_tables(par)


def _noisy_points(g, rng, n_rel, n_rand, sigma=1.2, flip=0.04):
    n = len(g["kx"])
    src = rng.integers(0, n, n_rel)
    flips = np.packbits(rng.random((n_rel, 256)) < flip, axis=1, bitorder="little")
    mp_desc = np.concatenate([g["desc"][src] ^ flips, rng.integers(0, 256, (n_rand, 32), dtype=np.uint8)])
    u = np.concatenate([g["kx"][src] + rng.normal(0, sigma, n_rel), rng.uniform(0, 752, n_rand)]).astype("f4")
    v = np.concatenate([g["ky"][src] + rng.normal(0, sigma, n_rel), rng.uniform(0, 480, n_rand)]).astype("f4")
    level = np.concatenate([np.clip(g["octave"][src] + rng.integers(0, 2, n_rel), 0, 7), rng.integers(0, 8, n_rand)]).astype("i4")
    return mp_desc, u, v, level, src


def random_scenes(O):
    out = []
    g, tab = _extract(O, 1)
    sf, is2 = tab["scale"], tab["inv_sigma2"]
    n = len(g["kx"])
    rng = np.random.default_rng(1)
    mp_desc, px, py, level, _ = _noisy_points(g, rng, 1200, 300, sigma=1.5, flip=0.05)
    view_cos = rng.uniform(0.99, 1.0, 1500).astype("f4")
    in_view = rng.random(1500) < 0.9; has_obs = rng.random(1500) < 0.95; occupied = rng.random(n) < 0.2
    for th in (1.0, 3.0):
        out.append(dict(name="random_projection_%g" % th, kind="projection", grid=g,
                        args=dict(scale_factors=sf, in_view=in_view, level=level, view_cos=view_cos, proj_x=px, proj_y=py, mp_desc=mp_desc,
                                  has_obs=has_obs, occupied=occupied, th=th, nnratio=0.8)))
    # a chain: 3000 points into one small region
    rng = np.random.default_rng(21)
    centre = np.array([g["kx"][n // 2], g["ky"][n // 2]])
    near = np.argsort((g["kx"] - centre[0]) ** 2 + (g["ky"] - centre[1]) ** 2)[:40]
    src = near[rng.integers(0, len(near), 3000)]
    out.append(dict(name="random_projection_chain", kind="projection", grid=g,
                    args=dict(scale_factors=sf, in_view=np.ones(3000, bool), level=np.clip(g["octave"][src] + rng.integers(0, 2, 3000), 0, 7),
                              view_cos=np.full(3000, 0.9, "f4"), proj_x=(centre[0] + rng.normal(0, 6, 3000)).astype("f4"),
                              proj_y=(centre[1] + rng.normal(0, 6, 3000)).astype("f4"),
                              mp_desc=g["desc"][src] ^ np.packbits(rng.random((3000, 256)) < 0.04, axis=1, bitorder="little"),
                              has_obs=rng.random(3000) < 0.7, occupied=np.zeros(n, bool), th=3.0, nnratio=0.8)))
    # frame to frame: frame 2 against itself shifted
    img = synth.frame(2)
    g1, _ = _extract(O, 2, img=img); g2, _ = _extract(O, 2, img=np.roll(img, (3, -5), axis=(0, 1)))
    rng = np.random.default_rng(4)
    n_last = len(g1["kx"])
    u = (g1["kx"] - 5 + rng.normal(0, 1.0, n_last)).astype("f4"); v = (g1["ky"] + 3 + rng.normal(0, 1.0, n_last)).astype("f4")
    valid = (rng.random(n_last) < 0.85) & (u >= 0) & (u <= 752) & (v >= 0) & (v <= 480)
    has_obs = rng.random(n_last) < 0.9
    for ori in (True, False):
        for th in (7.0, 40.0):
            out.append(dict(name="random_frame_%d_%g" % (ori, th), kind="frame", grid=g2,
                            args=dict(scale_factors=sf, valid=valid, u=u, v=v, last_octave=g1["octave"], last_angle=g1["angle"], mp_desc=g1["desc"],
                                      has_obs=has_obs, occupied=np.zeros(len(g2["kx"]), bool), th=th, check_ori=ori, orb_dist=100)))
    # the keyframe overload: has_obs all ones, ORBdist 64
    g, _ = _extract(O, 8)
    rng = np.random.default_rng(13)
    mp_desc, u, v, level, src = _noisy_points(g, rng, 800, 100, flip=0.12)
    kf_angle = rng.uniform(0, 360, 900).astype("f4")
    kf_angle[:800] = (g["angle"][src] + rng.normal(0, 3, 800)) % 360
    out.append(dict(name="random_frame_keyframe", kind="frame", grid=g,
                    args=dict(scale_factors=sf, valid=rng.random(900) < 0.9, u=u, v=v, last_octave=level, last_angle=kf_angle, mp_desc=mp_desc,
                              has_obs=np.ones(900, np.uint8), occupied=rng.random(len(g["kx"])) < 0.3, th=10.0, check_ori=True, orb_dist=64)))
    # initialisation: 2000 features, frame 3 against itself shifted
    img = synth.frame(3)
    g1, _ = _extract(O, 3, 2000, img); g2, _ = _extract(O, 3, 2000, np.roll(img, (6, 9), axis=(0, 1)))
    out.append(dict(name="random_init", kind="init", grid=g2,
                    args=dict(oct1=g1["octave"], desc1=g1["desc"], angle1=g1["angle"], prev_matched=np.stack([g1["kx"], g1["ky"]], 1), window=100,
                              nnratio=0.9, check_ori=True)))
    # Fuse with and without the chi2 test
    g, _ = _extract(O, 4)
    rng = np.random.default_rng(8)
    mp_desc, u, v, level, _ = _noisy_points(g, rng, 900, 200)
    valid = rng.random(1100) < 0.9
    for chi2 in (True, False):
        out.append(dict(name="random_fuse_%d" % chi2, kind="fuse", grid=g,
                        args=dict(scale_factors=sf, inv_level_sigma2=is2, valid=valid, u=u, v=v, level=level, mp_desc=mp_desc, th=3.0, chi2_check=chi2,
                                  accept_th=50)))
    # SearchByProjection(pKF, Scw)
    g, _ = _extract(O, 7)
    rng = np.random.default_rng(12)
    mp_desc, u, v, level, _ = _noisy_points(g, rng, 1400, 200)
    out.append(dict(name="random_sim3", kind="sim3", grid=g,
                    args=dict(scale_factors=sf, valid=rng.random(1600) < 0.9, u=u, v=v, level=level, mp_desc=mp_desc, observed=rng.random(1600) < 0.15,
                              matched=rng.random(len(g["kx"])) < 0.2, th=10.0)))
    # SearchBySim3
    g1, _ = _extract(O, 5); g2, _ = _extract(O, 6)
    rng = np.random.default_rng(11)
    n1, n2 = len(g1["kx"]), len(g2["kx"])
    p12 = rng.integers(0, n2, n1)
    mp1 = g2["desc"][p12] ^ np.packbits(rng.random((n1, 256)) < 0.05, axis=1, bitorder="little")
    u1 = (g2["kx"][p12] + rng.normal(0, 1.0, n1)).astype("f4"); v1 = (g2["ky"][p12] + rng.normal(0, 1.0, n1)).astype("f4")
    l1 = np.clip(g2["octave"][p12] + rng.integers(0, 2, n1), 0, 7)
    p21 = rng.integers(0, n1, n2)
    inv = np.full(n2, -1); inv[p12] = np.arange(n1)
    p21 = np.where((rng.random(n2) < 0.7) & (inv >= 0), inv, p21)
    mp2 = g1["desc"][p21] ^ np.packbits(rng.random((n2, 256)) < 0.05, axis=1, bitorder="little")
    u2 = (g1["kx"][p21] + rng.normal(0, 1.0, n2)).astype("f4"); v2 = (g1["ky"][p21] + rng.normal(0, 1.0, n2)).astype("f4")
    l2 = np.clip(g1["octave"][p21] + rng.integers(0, 2, n2), 0, 7)
    out.append(dict(name="random_by_sim3", kind="by_sim3", grid1=g1, grid2=g2,
                    args=dict(sf1=sf, sf2=sf, valid1=rng.random(n1) < 0.9, u1=u1, v1=v1, level1=l1, mp_desc1=mp1, valid2=rng.random(n2) < 0.9, u2=u2,
                              v2=v2, level2=l2, mp_desc2=mp2, th=7.5)))
    # GetFeaturesInArea itself
    g, _ = _extract(O, 0)
    rng = np.random.default_rng(0)
    x = rng.uniform(-30, 780, 400); y = rng.uniform(-30, 510, 400); r = rng.choice([2.5, 4.0, 10.0, 25.0, 60.0], 400)
    mn = rng.integers(-1, 6, 400); mx = np.where(rng.random(400) < 0.3, -1, mn + rng.integers(0, 3, 400))
    out.append(dict(name="random_area", kind="area", grid=g,
                    args=dict(queries=[(np.float32(x[q]), np.float32(y[q]), np.float32(r[q]), int(mn[q]), int(mx[q])) for q in range(400)])))
    return out


def test_random_scenes_equal_the_oracle(oracle):
    """Two independent restatements of the reference agree on every decision of the existing random scenes."""
    decisions = 0
    for case in random_scenes(oracle):
        trace = {}
        got, want = norm(C.run_ref(case, trace=trace)), norm(run_oracle(oracle, case))
        assert got == want, case["name"]
        decisions += sum(len(x) for x in got if isinstance(x, list))
        print("%-26s %s" % (case["name"], ", ".join("%s=%d" % kv for kv in sorted(trace.items()))))
    assert decisions > 10000


WRONG = ["tie_lowest_index", "radius_inclusive", "ratio_any_level", "occupy_always", "clear_current_owner", "grid_floor", "bin_ties_late"]


@pytest.mark.parametrize("wrong", WRONG)
def test_wrong_variant_is_caught(ref_runs, wrong):
    """A mistake the hand-built cases let through would also pass in a kernel: every variant changes at least one case's output."""
    caught = [c["name"] for c in C.small_cases() if norm(C.run_ref(c, wrong=(wrong,))) != ref_runs[c["name"]][1]]
    print("%-20s caught by: %s" % (wrong, ", ".join(caught)))
    assert caught


def test_definition_stands_alone():
    """The definition consults neither the oracle nor the package."""
    import ast
    import inspect
    mods = set()
    for node in ast.walk(ast.parse(inspect.getsource(R))):
        if isinstance(node, ast.Import):
            mods |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or "").split(".")[0])
    assert mods == {"math", "numpy"}
