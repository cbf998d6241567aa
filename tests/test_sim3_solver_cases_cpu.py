"""The yardsticks of tests/test_sim3_solver_cases_gpu.py, checked without a device: ref.check32 against the float64 restatement and
against csrc/sim3_ransac_math.h compiled for the host, the conditions the size batch must meet in the float64 reference alone, the
closed-form sampling map over every legal triple, and the bounds of the special inputs against the study that measures them."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import sim3_solver_cases as cases
import sim3_solver_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _samples(p, draws):
    return np.array([ref.sample_indices(len(p["X1"]), d) for d in draws], "i4").reshape(-1, 3)


def test_check32_follows_the_float64_errors_outside_the_band():
    """One problem (N = 129, 65 hypotheses): float32 estimates (the float64 closed form, rounded) go through check32 and through the
    float64 ref.errors; outside pairs within a relative 1e-3 of a bound the flags are equal, and the float32 errors are within 1e-3 of
    the float64 ones wherever those are not tiny."""
    problems, draws = cases.size_batch(sizes=[129])
    p = problems[0]
    R, t, s, gap = ref.horn(p["X1"][_samples(p, draws[0])], p["X2"][_samples(p, draws[0])], p["fix_scale"])
    R, t, s = R.astype("f4"), t.astype("f4"), s.astype("f4")
    flags, e1, e2 = ref.check32(R, t, s, p)
    w1, w2 = ref.errors(R.astype("f8"), t.astype("f8"), s.astype("f8"), p["X1"], p["X2"], p["K1"], p["K2"])
    m1, m2 = p["max_err1"][None].astype("f8"), p["max_err2"][None].astype("f8")
    amb = (np.abs(w1 / m1 - 1) < 1e-3) | (np.abs(w2 / m2 - 1) < 1e-3)
    want = (w1 < m1) & (w2 < m2)
    assert flags.shape == (65, 129) and not ((flags != want) & ~amb).any()
    assert amb.sum() <= 1e-3 * amb.size
    assert want.sum() > 200 and (~want).sum() > 200
    for e, w in ((e1, w1), (e2, w2)):
        big = w > 1e-2
        assert big.sum() > 0.9 * big.size and (np.abs(e[big] / w[big] - 1) < 1e-3).all()


def test_size_batch_meets_its_conditions_in_the_float64_reference():
    """Conditions on the inputs, from the float64 reference alone: ambiguous pairs <= 1e-3 of all pairs, degenerate hypotheses <= 2 %;
    at N = 1025 and 2049 a planted hypothesis has inliers in every tile of 1024, at N = 2049 more than 1024 of them."""
    problems, draws = cases.size_batch()
    pairs = amb_n = deg_n = hyp_n = 0
    for k, (p, d) in enumerate(zip(problems, draws)):
        n = len(p["X1"])
        assert n == cases.SIZES[k] and ref.ransac_iterations(n, cases.PROB, cases.MIN_INLIERS, 65) == 65
        r = ref.evaluate(p, _samples(p, d))
        with np.errstate(all="ignore"):
            amb = (np.abs(r["e1"] / p["max_err1"][None].astype("f8") - 1) < 1e-3) | (np.abs(r["e2"] / p["max_err2"][None].astype("f8") - 1) < 1e-3)
        pairs += amb.size; amb_n += int(amb.sum()); deg_n += int((r["gap"] < 1e-3).sum()); hyp_n += len(r["gap"])
        if n > cases.TILE:
            per_tile = [r["inlier"][:, t0:t0 + cases.TILE].sum(1) for t0 in range(0, n, cases.TILE)]
            full = np.all([c > 0 for c in per_tile], 0)
            print("N = %d: most inliers %d, hypotheses with an inlier in every tile %d" % (n, r["inlier"].sum(1).max(), full.sum()))
            assert full[6] and r["inlier"][6].sum() > 0.5 * n
            if n == 2049:
                assert r["inlier"].sum(1).max() > cases.TILE
    print("ambiguous pairs %d of %d (%.4f %%), degenerate hypotheses %d of %d (%.2f %%)" % (amb_n, pairs, 100.0 * amb_n / pairs, deg_n, hyp_n, 100.0 * deg_n / hyp_n))
    assert pairs == 65 * sum(cases.SIZES) and hyp_n == 650
    assert amb_n <= 1e-3 * pairs and deg_n <= 0.02 * hyp_n


def test_smaller_batches_hold_the_same_solvers():
    problems, draws = cases.size_batch()
    for its in (64, 1):
        sub, d = cases.size_batch(its, [65, 1025])
        for j, k in enumerate((2, 8)):
            assert d.shape == (2, its, 3) and (d[j] == draws[k, :its]).all()
            for key in ("X1", "X2", "max_err1", "max_err2", "indices1"):
                assert sub[j][key].tobytes() == problems[k][key].tobytes()


@pytest.fixture(scope="module")
def host_math(tmp_path_factory):
    """tests/support/sim3_ransac_math_check.cpp: the header the kernel includes, compiled for the host with the library's floating-point
    switches -> run(problem, draws [H][3]) = dict(sample, R, t, s, count, inlier)"""
    exe = str(tmp_path_factory.mktemp("s3r") / "sim3_ransac_math_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                           os.path.join(ROOT, "tests", "support", "sim3_ransac_math_check.cpp"), "-o", exe])

    def run(p, d):
        n, H = len(p["X1"]), len(d)
        blob = (np.array([n, int(p["fix_scale"]), H], "i4").tobytes() + p["K1"].astype("f4").tobytes() + p["K2"].astype("f4").tobytes()
                + p["X1"].astype("f4").tobytes() + p["X2"].astype("f4").tobytes() + p["max_err1"].astype("f4").tobytes()
                + p["max_err2"].astype("f4").tobytes() + np.ascontiguousarray(d, "i4").tobytes())
        out = subprocess.run([exe], input=blob, capture_output=True, timeout=120)
        assert out.returncode == 0, out.stderr
        buf = out.stdout
        sample = np.frombuffer(buf, "i4", 3 * H, 0).reshape(H, 3); rts = np.frombuffer(buf, "f4", 13 * H, 12 * H).reshape(H, 13)
        count = np.frombuffer(buf, "i4", H, 64 * H); inl = np.frombuffer(buf, "u1", H * n, 68 * H).reshape(H, n).astype(bool)
        assert len(buf) == 68 * H + H * n
        return dict(sample=sample, rts=rts, R=rts[:, :9].reshape(H, 3, 3), t=rts[:, 9:12], s=rts[:, 12], count=count, inlier=inl)
    return run


def _replay_holds(p, h):
    flags, _, _ = ref.check32(h["R"], h["t"], h["s"], p)
    assert (flags == h["inlier"]).all(), np.argwhere(flags != h["inlier"])[:5]
    assert (h["count"] == h["inlier"].sum(1)).all()


def test_check32_replays_the_math_header_bit_for_bit(host_math):
    """What the kernel's header computes on the host for (R, t, s), check32 reproduces from those (R, t, s): every flag of every
    hypothesis of the N = 65 (fixed scale), 1025 and 2049 solvers, of the degenerate solver and of the identity and half-turn ones."""
    problems, draws = cases.size_batch(sizes=[65, 1025, 2049])
    runs = list(zip(problems, draws)) + [(p, d[0]) for p, d in (cases.degenerate(), cases.identity(False), cases.identity(True), cases.half_turn())]
    for p, d in runs:
        h = host_math(p, d)
        assert (h["sample"] == _samples(p, d)).all()
        _replay_holds(p, h)
        if p["fix_scale"]:
            assert (h["s"] == 1.0).all()


def test_degenerate_solver_on_the_host(host_math):
    """The promises of the code comments on csrc/sim3_ransac_math.h, held on the host: coincident samples give s = NaN (frame 2) or
    s = 0 (frame 1) and no inlier at all; a collinear sample still gives a unit rotation; z = 0, a bound of 0 and a NaN bound are
    inliers of no hypothesis; a bound of +inf does not keep a correspondence out."""
    p, draws = cases.degenerate()
    h = host_math(p, draws[0])
    assert (h["sample"][:3] == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]).all()
    assert np.isnan(h["s"][0]) and h["s"][1] == 0.0
    assert (h["R"][:2] == np.eye(3, dtype="f4")).all()                       # M = 0: no rotation is applied, the quaternion stays (1, 0, 0, 0)
    assert h["count"][0] == 0 and h["count"][1] == 0 and not h["inlier"][:2].any()
    R = h["R"][2].astype("f8")
    assert np.isfinite(h["rts"][2]).all() and np.abs(R @ R.T - np.eye(3)).max() < 1e-6
    for k in (9, 10, 12, 14):
        assert not h["inlier"][:, k].any(), k
    assert h["inlier"][:, 13].any() and h["count"].max() > cases.MIN_INLIERS
    flags, e1, e2 = ref.check32(h["R"], h["t"], h["s"], p)
    assert np.isnan(e1[0]).all() and np.isnan(e2[1]).all()


def test_identity_and_half_turn_on_the_host(host_math):
    """X1 = X2: the header returns R = I exactly for every sample that spans a triangle and every correspondence is an inlier."""
    for fix in (False, True):
        p, draws = cases.identity(fix)
        h = host_math(p, draws[0])
        ok = cases.non_collinear(p, h["sample"])
        assert ok.sum() >= 60 and (h["R"][ok] == np.eye(3, dtype="f4")).all() and (h["count"][ok] == cases.SPECIAL_N).all()
    p, draws = cases.half_turn()
    h = host_math(p, draws[0])
    ok = cases.non_collinear(p, h["sample"])
    assert ok.sum() >= 60 and (h["count"][ok] == cases.SPECIAL_N).all()


def test_sampling_map_over_every_legal_triple(host_math):
    """s3r_sample (the closed form the kernel uses instead of the list) against the list simulation for all N (N-1) (N-2) triples of
    N = 3 .. 9, and the three indices are distinct."""
    for n in range(3, 10):
        rng = np.random.default_rng(n)
        p = ref.make_solver_problem(rng, n, 0.0, False)
        t = cases.all_triples(n)
        h = host_math(p, t)
        assert len(t) == n * (n - 1) * (n - 2) and (h["sample"] == _samples(p, t)).all()
        assert all(len(set(s)) == 3 for s in h["sample"].tolist()) and h["sample"].min() == 0 and h["sample"].max() == n - 1


def test_exhaustive_batch_covers_every_triple():
    problems, draws = cases.exhaustive_batch()
    its = [ref.ransac_iterations(n, cases.PROB, cases.EXHAUSTIVE_MIN_INLIERS, cases.EXHAUSTIVE_MAX_ITS) for n in cases.EXHAUSTIVE_SIZES]
    assert its == [123, 210, 210, 210, 210]
    for n, d, h in zip(cases.EXHAUSTIVE_SIZES, draws, its):
        assert len(set(map(tuple, d[:h].tolist())) & set(map(tuple, cases.all_triples(n).tolist()))) == n * (n - 1) * (n - 2)


def test_special_bounds_are_four_times_the_study():
    """tests/test_sim3_solver_cases_gpu.py states its bounds for the identity and half-turn solvers as 4 x what tools/sim3_ransac_study.py
    prints (three digits); this runs the study and holds the stated values to it."""
    spec = importlib.util.spec_from_file_location("sim3_ransac_study", os.path.join(ROOT, "tools", "sim3_ransac_study.py"))
    study = importlib.util.module_from_spec(spec); spec.loader.exec_module(study)
    with np.errstate(all="ignore"):
        measured = study.study_special()
    for name, stated in cases.SPECIAL_MEASURED.items():
        for got, want in zip(measured[name], stated):
            assert float("%.3g" % got) == want, (name, got, want)
