"""k_sim3_ransac at the edges of its design (tests/sim3_solver_cases.py): correspondence counts on the 64-bit mask-word edges, on the
edges of the 1024-correspondence LDS tile and past two tiles, 64 / 65 / 1 hypotheses per solver (one workgroup, one plus one, a
lone lane), every legal draw triple of N = 3 .. 7, and degenerate, identity and half-turn inputs.

The flags are held to an exact replay: ref.check32 evaluates :305-348 in float32 in the reference's operation order from the
(R, t, s) the kernel itself stored, and must reproduce every flag of every hypothesis -- degenerate ones included, no ambiguity band.
tests/test_sim3_solver_cases_cpu.py holds that replay to the float64 restatement and to the kernel's header compiled for the host.

Inputs, from the float64 reference alone (CPU, seed 41): 78 ambiguous pairs of 370,305 (0.021 %), 1 degenerate hypothesis of 650
(0.15 %); the planted hypothesis 6 has an inlier in every tile at N = 1025 (most inliers 650) and N = 2049 (most inliers 1213).

Bounds of the identity and half-turn solvers: 4 x the float32-against-float64 deviation of the closed form that
tools/sim3_ransac_study.py (study_special) prints for these inputs, over samples that span a triangle:
                          max |dR|    max |dt| / max(1, |t|inf)   max |ds| / s
  identity, free scale    0           4.77e-07                    5.96e-08      -> 0, 1.908e-06, 2.384e-07
  identity, fixed scale   0           0                           0             -> exact
  half turn               2.05e-06    2.39e-06                    8.8e-08       -> 8.2e-06, 9.56e-06, 3.52e-07
(at X1 = X2 the only rounding is the one of the scale's two sums, :278-292; R = I and, with the scale fixed, t = 0 come out exactly)."""

import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.sim3solver import Sim3Solver
import sim3_solver_cases as cases
import sim3_solver_ref as ref

pytestmark = pytest.mark.gpu

PROB, MIN_INLIERS = cases.PROB, cases.MIN_INLIERS
TOL = {name: tuple(4.0 * v for v in m) for name, m in cases.SPECIAL_MEASURED.items()}


def _solver(ctx, problems, draws, min_inliers=MIN_INLIERS, max_its=65):
    s = Sim3Solver(draws=draws, ctx=ctx, **ref.flatten(problems))
    s.SetRansacParameters(PROB, min_inliers, max_its)
    return s


def _raw(s, k, fill=0xFF):
    """ccm_sim3_solver_hypotheses of solver k into buffers prefilled with `fill`: sample, count, rts, mask words as the library copies them"""
    s._ensure()
    n = int(s.first[k + 1] - s.first[k]); words = (n + 63) // 64
    H = s.lib.ccm_sim3_solver_hypotheses(s._handle, int(k), None, None, None, None)
    assert H >= 0
    sample = np.full((H, 3), fill, "i4"); count = np.full(H, fill, "i4"); rts = np.full((H, 13), np.float32(7.5)); mask = np.full((H, words), 0xFFFFFFFFFFFFFFFF, "u8")
    assert s.lib.ccm_sim3_solver_hypotheses(s._handle, int(k), _lib.ptr(sample), _lib.ptr(count), _lib.ptr(rts), _lib.ptr(mask)) == H
    return dict(sample=sample, count=count, rts=rts, mask=mask)


def _unpack(mask, n):
    """all 64 bits of every word -> [H][words * 64] bool"""
    return ((mask[:, :, None] >> np.arange(64, dtype="u8")[None, None]) & np.uint64(1)).astype(bool).reshape(len(mask), -1)


def _exact_replay(p, h, where):
    """every flag from the stored (R, t, s); the count is the mask's popcount"""
    flags, _, _ = ref.check32(h["R"], h["t"], h["s"], p)
    bad = flags != h["inlier"]
    assert not bad.any(), (where, int(bad.sum()), np.argwhere(bad)[:5])
    assert (h["count"] == h["inlier"].sum(1)).all(), where


@pytest.fixture(scope="module")
def sizes(ctx):
    problems, draws = cases.size_batch(65)
    s = _solver(ctx, problems, draws)
    hyps = [s.hypotheses(k) for k in range(len(problems))]
    raws = [_raw(s, k) for k in range(len(problems))]
    refs = [ref.evaluate(p, h["sample"]) for p, h in zip(problems, hyps)]
    s.close()
    return problems, draws, hyps, raws, refs


def test_sizes_every_solver_evaluates_a_block_plus_one(sizes):
    problems, draws, hyps, raws, refs = sizes
    assert [len(p["X1"]) for p in problems] == cases.SIZES and sum(p["fix_scale"] for p in problems) >= 2
    for k, (p, h) in enumerate(zip(problems, hyps)):
        n = len(p["X1"])
        assert len(h["count"]) == cases.HPB + 1 and h["inlier"].shape == (65, n)
        assert (h["sample"] == [ref.sample_indices(n, d) for d in draws[k]]).all(), k
        if p["fix_scale"]:
            assert (h["s"] == 1.0).all()


def test_sizes_exact_replay_of_every_flag(sizes):
    problems, draws, hyps, raws, refs = sizes
    for k, (p, h) in enumerate(zip(problems, hyps)):
        _exact_replay(p, h, k)


def test_sizes_raw_words_hold_the_flags_and_nothing_above_n(sizes):
    """The words as the C entry returns them: bit i % 64 of word i / 64 is correspondence i, the padding bits of the last word are 0."""
    problems, draws, hyps, raws, refs = sizes
    for k, (p, h, raw) in enumerate(zip(problems, hyps, raws)):
        n = len(p["X1"])
        bits = _unpack(raw["mask"], n)
        assert raw["mask"].shape == (65, (n + 63) // 64)
        assert (bits[:, :n] == h["inlier"]).all() and not bits[:, n:].any(), (k, n)
        assert (raw["count"] == bits.sum(1)).all() and (raw["sample"] == h["sample"]).all()
        assert raw["rts"].tobytes() == np.concatenate([h["R"].reshape(65, 9), h["t"], h["s"][:, None]], 1).tobytes()
    assert {65, 1025} <= {len(p["X1"]) for p in problems}


def test_sizes_flags_counts_and_estimates_against_float64(sizes):
    """The older module's comparisons with their bounds: flags equal outside ambiguous pairs (err / maxErr within a relative 1e-3 of 1)
    and degenerate hypotheses (eigenvalue gap below 1e-3), counts up to the ambiguous ones, R within 1e-3, t within 1e-3 max(1, |t|inf),
    s within a relative 1e-5; ambiguous pairs <= 1e-3 of all pairs, degenerate hypotheses <= 2 %."""
    problems, draws, hyps, raws, refs = sizes
    pairs = amb_n = deg_n = hyp_n = 0; worst = np.zeros(3)
    for k, (p, h, r) in enumerate(zip(problems, hyps, refs)):
        with np.errstate(all="ignore"):
            amb = (np.abs(r["e1"] / p["max_err1"][None].astype("f8") - 1) < 1e-3) | (np.abs(r["e2"] / p["max_err2"][None].astype("f8") - 1) < 1e-3)
        deg = r["gap"] < 1e-3; ok = ~deg
        pairs += amb.size; amb_n += int(amb.sum()); deg_n += int(deg.sum()); hyp_n += len(deg)
        wrong = (h["inlier"] != r["inlier"]) & ~amb & ok[:, None]
        assert not wrong.any(), (k, np.argwhere(wrong)[:5])
        assert (np.abs(h["count"] - r["inlier"].sum(1))[ok] <= amb.sum(1)[ok]).all(), k
        dR = np.abs(h["R"] - r["R"]).max((1, 2))[ok]
        dt = (np.abs(h["t"] - r["t"]).max(1) / np.maximum(1, np.abs(r["t"]).max(1)))[ok]
        ds = (np.abs(h["s"] - r["s"]) / np.abs(r["s"]))[ok]
        worst = np.maximum(worst, [dR.max(), dt.max(), ds.max()])
        assert dR.max() <= 1e-3 and dt.max() <= 1e-3 and ds.max() <= 1e-5, (k, dR.max(), dt.max(), ds.max())
    print("ambiguous pairs %d of %d (%.4f %%), degenerate hypotheses %d of %d (%.2f %%)" % (amb_n, pairs, 100.0 * amb_n / pairs, deg_n, hyp_n, 100.0 * deg_n / hyp_n))
    print("worst |dR| %.3g, |dt| %.3g, |ds|/s %.3g" % tuple(worst))
    assert pairs == 65 * sum(cases.SIZES) and hyp_n == 650
    assert amb_n <= 1e-3 * pairs and deg_n <= 0.02 * hyp_n


def test_sizes_every_tile_is_populated(sizes):
    """Past one tile the planted hypotheses (three correct matches each) have inliers in every tile of 1024 -- also in the last, which
    holds a single correspondence -- and at N = 2049 more than 1024 in all, so a count that restarted per tile or a word written to
    the first tile's offset could not go unseen."""
    problems, draws, hyps, raws, refs = sizes
    seen = 0
    for p, h in zip(problems, hyps):
        n = len(p["X1"])
        if n <= cases.TILE:
            continue
        seen += 1
        per_tile = np.array([h["inlier"][:, t0:t0 + cases.TILE].sum(1) for t0 in range(0, n, cases.TILE)])
        print("N = %d: most inliers %d, inliers per tile of hypothesis 6: %s" % (n, h["count"].max(), per_tile[:, 6].tolist()))
        assert len(per_tile) == (n + cases.TILE - 1) // cases.TILE and (per_tile[:, 6] > 0).all()
        assert h["count"][6] == per_tile[:, 6].sum() > 0.5 * n
        assert (per_tile.min(0) > 0).sum() >= 2
        if n == 2049:
            assert h["count"].max() > cases.TILE
    assert seen == 2


@pytest.mark.parametrize("max_its", [65, 64, 1])
def test_alone_or_in_a_batch_the_rows_are_identical_bytes(ctx, sizes, max_its):
    """N = 65 and N = 1025 created alone, as a batch of two and twice over, at 65, 64 (exactly one workgroup) and 1 hypotheses: the rows
    are the bytes of the ten-solver batch's first rows (a hypothesis depends on nothing but its own draw); the exact replay and
    the zero padding bits hold on each."""
    problems, draws, hyps, raws, refs = sizes
    sub, d = cases.size_batch(max_its, [65, 1025])
    pair = _solver(ctx, sub, d, max_its=max_its)
    again = _solver(ctx, sub, d, max_its=max_its)
    for j, k in enumerate((2, 8)):
        n = len(sub[j]["X1"])
        alone = _solver(ctx, sub[j:j + 1], d[j:j + 1], max_its=max_its)
        got = [_raw(pair, j), _raw(again, j), _raw(alone, 0)]
        for g in got:
            assert len(g["count"]) == max_its
            for key in ("sample", "count", "rts", "mask"):
                assert g[key].tobytes() == raws[k][key][:max_its].tobytes(), (n, key)
            assert not _unpack(g["mask"], n)[:, n:].any()
        _exact_replay(sub[j], alone.hypotheses(0), (n, max_its))
        alone.close()
    pair.close(); again.close()


def _estimate_bytes(s, k):
    """ccm_sim3_solver_estimate into float32 buffers: the bytes of R, t, s"""
    R = np.zeros(9, "f4"); t = np.zeros(3, "f4"); sc = np.zeros(1, "f4")
    assert s.lib.ccm_sim3_solver_estimate(s._handle, int(k), _lib.ptr(R), _lib.ptr(t), _lib.ptr(sc)) == 0
    return R.tobytes() + t.tobytes() + sc.tobytes()


def _ref_solver(p, h, min_inliers, max_its):
    n = len(p["X1"])
    return ref.RefSolver(n, p["n1"], p["indices1"], h["count"], h["inlier"], min_inliers, ref.ransac_iterations(n, PROB, min_inliers, max_its))


def _bookkeeping_replays(s, k, p, h, step, min_inliers=MIN_INLIERS, max_its=65):
    """iterate / find of solver k call by call against ref.RefSolver fed with the device's counts and masks -> returns seen"""
    rs = _ref_solver(p, h, min_inliers, max_its)
    n = len(p["X1"]); returns = 0
    for call in range(max_its + 2):
        if step == "find":
            T, vb, nin = s.find(k); rh, rvb, rn = rs.find(); no_more = rno = rs.mnIterations >= rs.mRansacMaxIts
        else:
            T, no_more, vb, nin = s.iterate(k, step); rh, rno, rvb, rn = rs.iterate(step)
        assert (T is not None) == (rh is not None) and no_more == rno and nin == rn, (k, call)
        assert len(vb) == p["n1"] and (vb == rvb).all(), (k, call)
        if rh is not None:
            returns += 1
            scattered = np.zeros(p["n1"], bool); scattered[p["indices1"][h["inlier"][rh]]] = True      # :179-181 over all words
            assert (vb == scattered).all() and vb.sum() == nin == h["count"][rh]
            for t0 in range(0, n, 64):                                       # word by word: each word's correspondences land where mvnIndices1 says
                assert (vb[p["indices1"][t0:t0 + 64]] == h["inlier"][rh, t0:t0 + 64]).all(), (k, call, t0 // 64)
            T12 = np.eye(4, dtype="f4"); T12[:3, :3] = h["s"][rh] * h["R"][rh]; T12[:3, 3] = h["t"][rh]
            assert T.tobytes() == T12.tobytes()
        st = s.state(k)
        assert st["iterations"] == rs.mnIterations and st["best_hypothesis"] == rs.best and st["best_inliers"] == rs.mnBestInliers
        if rs.best >= 0:                                                     # the getters return the stored bytes (NaN included)
            assert s.GetEstimatedRotation(k).tobytes() == h["R"][rs.best].tobytes() and s.GetEstimatedTranslation(k).tobytes() == h["t"][rs.best].tobytes()
            assert _estimate_bytes(s, k) == h["R"][rs.best].tobytes() + h["t"][rs.best].tobytes() + h["s"][rs.best].tobytes()
        else:
            assert s.GetEstimatedRotation(k) is None
        if no_more:
            break
    assert no_more
    return returns


@pytest.mark.parametrize("step", [5, "find"])
def test_sizes_bookkeeping_replays_iterate_and_find(ctx, sizes, step):
    """iterate(k, 5) and find(k) on the N = 1025 and N = 2049 solvers: vbInliers is the mask scattered through mvnIndices1, words 16 to
    32 included."""
    problems, draws, hyps, raws, refs = sizes
    s = _solver(ctx, problems, draws)
    for k in (8, 9):
        assert len(problems[k]["X1"]) in (1025, 2049)
        returns = _bookkeeping_replays(s, k, problems[k], hyps[k], step)
        assert returns >= 1
        best = int(np.argmax(hyps[k]["count"]))
        assert hyps[k]["inlier"][best, 1024:].any()
    s.close()


def test_exhaustive_sampling(ctx):
    """N = 3 .. 7 at MinInliers 1 and MaxIterations 210: 123, 210, 210, 210, 210 hypotheses whose first rows are every legal draw
    triple; the kernel's closed-form map gives the list simulation's sample for each, three distinct indices."""
    problems, draws = cases.exhaustive_batch()
    s = _solver(ctx, problems, draws, cases.EXHAUSTIVE_MIN_INLIERS, cases.EXHAUSTIVE_MAX_ITS)
    rows = []
    for k, (n, p) in enumerate(zip(cases.EXHAUSTIVE_SIZES, problems)):
        h = s.hypotheses(k)
        rows.append(len(h["count"]))
        triples = cases.all_triples(n)
        assert (draws[k, :len(triples)] == triples).all() and len(triples) == n * (n - 1) * (n - 2) <= len(h["count"])
        want = np.array([ref.sample_indices(n, d) for d in draws[k, :len(h["count"])]])
        assert (h["sample"] == want).all(), (n, np.argwhere(h["sample"] != want)[:5])
        assert all(len(set(t)) == 3 for t in h["sample"].tolist()) and h["sample"].min() >= 0 and h["sample"].max() == n - 1
        _exact_replay(p, h, n)
    assert rows == [123, 210, 210, 210, 210]
    s.close()


def test_degenerate_solver(ctx):
    """tests/sim3_solver_cases.degenerate: the exact replay holds on every row, NaN and inf rows included; z = 0 and bounds of 0 and NaN
    are inliers of no hypothesis; the two coincident samples count 0 (s = NaN and s = 0: confirmed on the host header by the CPU
    module); iterate and find replay the reference class; the getters return the stored bytes."""
    p, draws = cases.degenerate()
    s = _solver(ctx, [p], draws)
    h = s.hypotheses(0); raw = _raw(s, 0)
    assert len(h["count"]) == 65 and (h["sample"][:3] == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]).all()
    _exact_replay(p, h, "degenerate")
    bits = _unpack(raw["mask"], 70)
    assert (bits[:, :70] == h["inlier"]).all() and not bits[:, 70:].any()
    for k in (9, 10, 12, 14):
        assert not h["inlier"][:, k].any(), k
    assert h["inlier"][:, 13].any()
    flags, e1, e2 = ref.check32(h["R"], h["t"], h["s"], p)
    assert np.isnan(h["s"][0]) and h["s"][1] == 0.0 and (h["R"][:2] == np.eye(3, dtype="f4")).all()
    assert h["count"][0] == flags[0].sum() == 0 and h["count"][1] == flags[1].sum() == 0
    assert np.isfinite(raw["rts"][2]).all() and np.abs(h["R"][2].astype("f8") @ h["R"][2].astype("f8").T - np.eye(3)).max() < 1e-6
    for step in (1, 5, "find"):
        t = _solver(ctx, [p], draws)
        returns = _bookkeeping_replays(t, 0, p, h, step)
        assert returns >= 1
        t.close()
    # hypothesis 0 (count 0 >= mnBestInliers 0) becomes the best first: the getters hand out its NaN as stored
    t = _solver(ctx, [p], draws)
    t.iterate(0, 1)
    assert t.state(0)["best_hypothesis"] == 0 and np.isnan(t.GetEstimatedScale(0))
    assert _estimate_bytes(t, 0) == raw["rts"][0].tobytes()
    t.close(); s.close()


def _estimates_within(p, h, tol, name):
    ok = cases.non_collinear(p, h["sample"])
    R, t, sc, gap = ref.horn(p["X1"][h["sample"]], p["X2"][h["sample"]], p["fix_scale"])
    dR = np.abs(h["R"] - R).max((1, 2))[ok]
    dt = (np.abs(h["t"] - t).max(1) / np.maximum(1, np.abs(t).max(1)))[ok]
    ds = (np.abs(h["s"] - sc) / np.abs(sc))[ok]
    print("%s: %d samples, worst |dR| %.3g (bound %.3g), |dt| %.3g (%.3g), |ds|/s %.3g (%.3g)" % (name, ok.sum(), dR.max(), tol[0], dt.max(), tol[1], ds.max(), tol[2]))
    assert ok.sum() >= 60 and gap[ok].min() >= 1e-3
    assert dR.max() <= tol[0] and dt.max() <= tol[1] and ds.max() <= tol[2], (name, dR.max(), dt.max(), ds.max())
    return ok


@pytest.mark.parametrize("fix_scale", [False, True])
def test_identity_solver(ctx, fix_scale):
    """X1 = X2: zero rotation, every `apr == 0` branch of the first row of the Jacobi.  R, t, s against the float64 closed form within
    the module docstring's bounds for every sample that spans a triangle; every correspondence is an inlier of each."""
    name = "identity, fixed scale" if fix_scale else "identity, free scale"
    p, draws = cases.identity(fix_scale)
    s = _solver(ctx, [p], draws)
    h = s.hypotheses(0)
    ok = _estimates_within(p, h, TOL[name], name)
    _exact_replay(p, h, name)
    assert (h["count"][ok] == cases.SPECIAL_N).all() and h["inlier"][ok].all()
    if fix_scale:
        assert (h["s"] == 1.0).all()
    s.close()


def test_half_turn_solver(ctx):
    """X1 = diag(-1, -1, 1) X2 + t0: the quaternion's w is 0."""
    p, draws = cases.half_turn()
    s = _solver(ctx, [p], draws)
    h = s.hypotheses(0)
    ok = _estimates_within(p, h, TOL["half turn"], "half turn")
    _exact_replay(p, h, "half turn")
    assert (np.abs(np.trace(h["R"][ok].astype("f8"), axis1=1, axis2=2) + 1) < 1e-4).all()                   # 1 + 2 cos(pi)
    assert (h["count"][ok] == cases.SPECIAL_N).all()
    s.close()
