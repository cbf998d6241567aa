"""Batched PnPsolver (src/PnPSolver.cpp) on the GPU: k_pnp_hypotheses and k_pnp_refine against tests/pnp_solver_ref.py.

Per-hypothesis agreement with the reference is not definable (the pose depends on the SVD's arbitrary null basis; DESIGN.md
"PnPsolver"), so the kernels are held to two things: the inlier flags and counts are the EXACT check_inliers of the double pose
the library reports, and that pose agrees with the float64 restatement fed with the library's own tapped (control points, basis),
within a tolerance taken from the restatement's own sensitivity (pnp_solver_ref.pose_tolerance / pose_agrees).

Shapes, the smallest at which the kernels can go wrong: N = 3 (below min_set: nothing evaluated), 4 (minInliers == N: one
iteration), 9, 63 / 64 / 65 (mask word edge), 1025 (one past the LDS tile); 1, 16 (one block of hypotheses) and 17 hypotheses per
solver; min_set 4 and 5; batches of 0, 1 and 7 solvers."""
import ctypes as C

import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.pnpsolver import PNP_HPB, PNP_TILE, PnPSolver, make_draws
import pnp_solver_ref as ref

pytestmark = pytest.mark.gpu

PROB, MIN_INLIERS, EPS, TH2 = 0.99, 4, 0.4, 5.991
#        N, wrong-match share
SHAPES = [(3, 0.0), (4, 0.0), (9, 0.0), (63, 0.3), (64, 0.3), (65, 0.3), (PNP_TILE + 1, 0.3)]
#          min_set, max_iterations, reserve: 16 = one block of hypotheses, 16 + 1 = one block + 1
BATCHES = {"A": (4, PNP_HPB, 0), "B": (5, PNP_HPB, 1)}


def _problems(seed):
    rng = np.random.default_rng(seed)
    return [ref.make_problem(rng, n, wrong) for n, wrong in SHAPES]


def _draws(problems, rows, min_set, seed):
    rng = np.random.default_rng(seed)
    sizes = [len(p["P2D"]) for p in problems]
    draws = make_draws(rng, sizes, rows, min_set)
    for k, n in enumerate(sizes):                       # the corners of :178-192: the last element, repeated values, position 0
        if n >= 9:
            draws[k, 0] = [n - 1 - i for i in range(min_set)]; draws[k, 1] = 0
            draws[k, 2] = [n - 2, n - 2, 0, 0, 1][:min_set]; draws[k, 3] = 1
    return draws


def _solver(ctx, problems, draws, min_set, max_its, reserve, detail=True, min_inliers=MIN_INLIERS):
    s = PnPSolver(draws=draws, reserve=reserve, detail=detail, ctx=ctx, **ref.flatten(problems))
    s.SetRansacParameters(PROB, min_inliers, max_its, min_set, EPS, TH2)
    return s


@pytest.fixture(scope="module")
def batches(ctx):
    out = {}
    for name, (min_set, max_its, reserve) in BATCHES.items():
        problems = _problems(7)
        draws = _draws(problems, max_its + reserve, min_set, 11)
        s = _solver(ctx, problems, draws, min_set, max_its, reserve)
        hyps = [s.hypotheses(k) for k in range(len(problems))]
        refs = [s.refinements(k) for k in range(len(problems))]
        states = [s.state(k) for k in range(len(problems))]
        s.close()
        out[name] = dict(problems=problems, draws=draws, hyps=hyps, refs=refs, states=states, min_set=min_set, max_its=max_its, reserve=reserve)
    return out


def test_hypothesis_rows_follow_set_ransac_parameters(batches):
    for name, b in batches.items():
        for (n, _), h, st in zip(SHAPES, b["hyps"], b["states"]):
            mi, its, _ = ref.ransac_parameters(n, PROB, MIN_INLIERS, b["max_its"], b["min_set"], EPS)
            assert (st["min_inliers"], st["max_iterations"]) == (mi, its), (name, n)
            assert len(h["count"]) == (its + b["reserve"] if n >= mi else 0), (name, n)
    a = [len(h["count"]) for h in batches["A"]["hyps"]]
    assert a[0] == 0 and a[1] == 1 and a[3:] == [PNP_HPB] * 4            # N = 3: none; N = 4: minInliers == N, one iteration
    assert [len(h["count"]) for h in batches["B"]["hyps"]][3:] == [PNP_HPB + 1] * 4


def test_sampling_is_the_reference_swap_with_last(batches):
    seen_last = seen_repeat = 0
    for name, b in batches.items():
        for k, (p, h) in enumerate(zip(b["problems"], b["hyps"])):
            n = len(p["P2D"])
            for i, smp in enumerate(h["sample"]):
                assert list(smp) == ref.sample_indices(n, b["draws"][k, i]), (name, k, i)
                assert len(set(smp)) == b["min_set"]
                seen_last += int(b["draws"][k, i, 0] == n - 1); seen_repeat += int(len(set(b["draws"][k, i])) < b["min_set"])
    assert seen_last >= 8 and seen_repeat >= 16


def test_counts_and_masks_are_the_exact_check_inliers_of_the_reported_pose(batches):
    rows = inl = 0
    for name, b in batches.items():
        for k, (p, h, r) in enumerate(zip(b["problems"], b["hyps"], b["refs"])):
            for tap in (h, r):
                if len(tap["count"]) == 0:
                    continue
                want = ref.check_inliers(tap["Rt"], p["K"], p["P3Dw"], p["P2D"], ref.max_error(p["sigma2"], TH2))
                assert (tap["inlier"] == want).all(), (name, k, np.argwhere(tap["inlier"] != want)[:5])
                assert (tap["count"] == want.sum(1)).all(), (name, k)
                rows += len(want); inl += int(want.sum())
    assert rows >= 150 and inl >= 2000


def test_refinement_rows_are_the_records_of_the_counts(batches):
    n_rec = 0
    for name, b in batches.items():
        for k, (h, r, st) in enumerate(zip(b["hyps"], b["refs"], b["states"])):
            assert list(r["hyp"]) == ref.records(h["count"], st["min_inliers"]), (name, k)
            n_rec += len(r["hyp"])
    assert n_rec >= 12


def _check_poses(p, tap, sets, rng, tag):
    """tap rows against the restatement fed with their own tapped pair -> (checked, skipped)"""
    checked = skipped = 0
    K = p["K"].astype("f8")
    for i, idx in enumerate(sets):
        pw, us = p["P3Dw"][idx].astype("f8"), p["P2D"][idx].astype("f8")
        r, d = ref.pose_tolerance(rng, pw, us, K, tap["cws"][i], tap["basis"][i])
        if not np.isfinite(d) or d > 1e-3:
            skipped += 1
            continue
        checked += 1
        assert ref.pose_agrees(tap["R"][i], tap["t"][i], tap["which"][i], tap["rep_error"][i], r, d), \
            (tag, i, d, np.abs(tap["R"][i] - r["R"]).max(), tap["which"][i], r["which"], tap["rep_error"][i], r["rep_error"])
    return checked, skipped


def _tapped_pair_is_valid(p, tap, sets, tag):
    """cws[0] the centroid, the axes orthogonal with |axis|^2 = an eigenvalue of the covariance / n; the basis rows orthonormal
    eigenvectors of M^T M with the four smallest eigenvalues"""
    K = p["K"].astype("f8")
    for i, idx in enumerate(sets):
        pw, us = p["P3Dw"][idx].astype("f8"), p["P2D"][idx].astype("f8")
        cws, v = tap["cws"][i], tap["basis"][i]
        n = len(idx); c0 = pw.sum(0) / n
        scale = max(1.0, np.abs(pw).max())
        assert np.abs(cws[0] - c0).max() <= 1e-12 * scale, (tag, i)
        cov = (pw - c0).T @ (pw - c0) / n
        ax = cws[1:] - cws[0]
        lam = (ax ** 2).sum(1)
        assert np.abs(ax @ ax.T - np.diag(lam)).max() <= 1e-9 * lam.max(), (tag, i)
        assert np.abs(cov @ ax.T - ax.T * lam).max() <= 1e-9 * lam.max() * np.sqrt(lam.max()), (tag, i)
        assert np.abs(np.sort(lam) - np.linalg.eigvalsh(cov)).max() <= 1e-9 * lam.max(), (tag, i)
        M = ref.fill_M(ref.barycentric(pw, cws), us, K); A = M.T @ M; nA = np.linalg.norm(A, 2)
        mu = np.einsum("ij,jk,ik->i", v, A, v)
        assert np.abs(A @ v.T - v.T * mu).max() <= 1e-9 * nA, (tag, i)
        assert np.abs(v @ v.T - np.eye(4)).max() <= 1e-10, (tag, i)
        assert np.abs(np.sort(mu) - np.linalg.eigvalsh(A)[:4]).max() <= 1e-9 * nA, (tag, i)


def test_device_pose_agrees_with_the_restatement_fed_with_its_tapped_pair(batches):
    """Every hypothesis and every refinement of both batches.  The tolerance per row is max(1e-9, 100 d), d the restatement's own
    deviation under a 1e-11 perturbation of the basis; rows with d > 1e-3 or a non-finite restatement are skipped, at most 2 %."""
    rng = np.random.default_rng(5)
    checked = skipped = 0
    for name, b in batches.items():
        for k, (p, h, r) in enumerate(zip(b["problems"], b["hyps"], b["refs"])):
            sets_h = [list(s) for s in h["sample"]]
            sets_r = [np.flatnonzero(h["inlier"][hyp]) for hyp in r["hyp"]]
            for tap, sets, tag in ((h, sets_h, (name, k, "hyp")), (r, sets_r, (name, k, "refine"))):
                _tapped_pair_is_valid(p, tap, sets, tag)
                c, s = _check_poses(p, tap, sets, rng, tag)
                checked += c; skipped += s
    print("poses checked %d, skipped %d" % (checked, skipped))
    assert checked >= 150 and skipped <= 0.02 * (checked + skipped)


def test_device_pose_equals_the_host_entry_where_their_bases_agree(batches):
    """ccm_pnp_compute_pose is the same arithmetic through the host compiler.  Where host and device arrive at the same (control
    points, basis) to 1e-12, their poses agree within the tolerance rule; the share of such rows is printed (an order difference
    between the two eigen-solvers is legitimate and is covered by the test above)."""
    rng = np.random.default_rng(6)
    same = total = 0
    b = batches["A"]
    for k, (p, h) in enumerate(zip(b["problems"], b["hyps"])):
        for i, smp in enumerate(h["sample"][:6]):
            R, t, d = PnPSolver.compute_pose(p["P3Dw"][smp], p["P2D"][smp], p["K"], detail=True)
            total += 1
            if np.abs(d["cws"] - h["cws"][i]).max() <= 1e-12 * max(1, np.abs(d["cws"]).max()) and np.abs(d["basis"] - h["basis"][i]).max() <= 1e-12:
                same += 1
                r, dev = ref.pose_tolerance(rng, p["P3Dw"][smp].astype("f8"), p["P2D"][smp].astype("f8"), p["K"].astype("f8"), d["cws"], d["basis"])
                if np.isfinite(dev) and dev <= 1e-3:
                    assert ref.pose_agrees(R, t, d["which"], d["rep_error"], r, dev) and ref.pose_agrees(h["R"][i], h["t"][i], h["which"][i], h["rep_error"][i], r, dev)
    print("host and device share the basis in %d of %d rows" % (same, total))


def _ref_solver(p, h, r, st):
    by_mask = {h["inlier"][hyp].tobytes(): j for j, hyp in enumerate(r["hyp"])}

    def refine(mask):
        j = by_mask[np.asarray(mask).tobytes()]
        return int(r["count"][j]), r["inlier"][j]
    return ref.RefSolver(len(p["P2D"]), p["n1"], p["kp_index"], h["count"], h["inlier"], st["min_inliers"], st["max_iterations"], refine)


def _pose_of(name, h, r):
    kind, hyp = name
    return ref.tcw(r["Rt"][list(r["hyp"]).index(hyp)]) if kind == "refined" else ref.tcw(h["Rt"][hyp])


@pytest.mark.parametrize("step", [1, 5, PNP_HPB, "find"])
def test_bookkeeping_replays_iterate_exactly(ctx, step):
    """iterate driven 1, 5 and H at a time and through find() returns, call by call, what the literal reference class returns when it
    is fed the device's own counts, masks and refinements, with reserve = the step.  A solver is resumed after every return until it
    reports bNoMore -- or until a call would need hypotheses beyond the reserve (a return at or past mRansacMaxIts does not set
    bNoMore, and every further call draws up to `step` more): exactly there the library answers CCM_E_STATE and changes nothing."""
    min_set, max_its = 4, PNP_HPB
    reserve = 0 if step == "find" else step
    problems = _problems(7)
    s = _solver(ctx, problems, _draws(problems, max_its + reserve, min_set, 11), min_set, max_its, reserve)
    returns = {"refined": 0, "best": 0}; beyond = 0
    for k, p in enumerate(problems):
        h, r, st = s.hypotheses(k), s.refinements(k), s.state(k)
        rs = _ref_solver(p, h, r, st)
        H = len(h["count"])
        for call in range(60):
            if step == "find":
                T, vb, n = s.find(k); name, rvb, rn = rs.find(); no_more = True
            else:
                if H and max(st["max_iterations"], rs.mnIterations + step) > H:      # the literal loop would read past what was evaluated
                    before = s.state(k)
                    with pytest.raises(_lib.CcmError) as err:
                        s.iterate(k, step)
                    assert err.value.code == -7 and s.state(k) == before, (k, call)
                    beyond += 1; no_more = True
                    break
                T, no_more, vb, n = s.iterate(k, step); name, rno, rvb, rn = rs.iterate(step)
                assert no_more == rno, (k, call)
            assert (T is not None) == (name is not None) and n == rn, (k, call)
            assert len(vb) == p["n1"] and (vb == rvb).all(), (k, call)
            if name is not None:
                returns[name[0]] += 1
                assert (T == _pose_of(name, h, r)).all() and vb.sum() == n, (k, call)
            now = s.state(k)
            assert (now["iterations"], now["best_inliers"], now["best_hypothesis"]) == (rs.mnIterations, rs.mnBestInliers, rs.best), (k, call)
            if no_more:
                break
        assert no_more, k
        if step != "find" and H:                          # far beyond the reserve, whatever the state
            before = s.state(k)
            rc = s.lib.ccm_pnp_solver_iterate(s._handle, k, H + 1, C.byref(C.c_int32()), C.byref(C.c_int32()), None, C.byref(C.c_int32()), None)
            assert rc == -7 and s.state(k) == before, k
    print("step %s: returns %s, calls beyond the reserve %d" % (step, returns, beyond))
    assert returns["refined"] >= 3, returns
    s.close()


def test_end_to_end_find_recovers_the_pose(ctx):
    """N = 200 with 70 % true matches, the reference's default parameters: find reports a pose, within 5 x the error of the
    restatement's EPnP on the problem's true inlier set (the margin allows a refined set that is not exactly the true one)."""
    rng = np.random.default_rng(17)
    problems = [ref.make_problem(rng, 200, 0.3) for _ in range(3)]
    for p in problems:
        assert (~p["bad"]).sum() >= 120
    reserve = 5
    draws = make_draws(rng, [200] * 3, 300 + reserve, 4)
    s = PnPSolver(draws=draws, reserve=reserve, ctx=ctx, **ref.flatten(problems))          # SetRansacParameters() defaults
    for k, p in enumerate(problems):
        T, vb, n = s.find(k)
        assert T is not None and n > s.state(k)["min_inliers"], k
        good = ~p["bad"]
        e = ref.epnp(p["P3Dw"][good].astype("f8"), p["P2D"][good].astype("f8"), p["K"].astype("f8"))
        eR, et = np.abs(e["R"] - p["R"]).max(), np.abs(e["t"] - p["t"]).max()
        dR, dt = np.abs(T[:3, :3] - p["R"]).max(), np.abs(T[:3, 3] - p["t"]).max()
        print("solver %d: %d inliers, |dR| %.3g (bound %.3g), |dt| %.3g (bound %.3g)" % (k, n, dR, 5 * eR, dt, 5 * et))
        assert dR <= 5 * eR + 1e-6 and dt <= 5 * et + 1e-6, k                        # 1e-6: the returned pose is float32
        assert (vb[p["kp_index"]] & good).sum() >= 0.9 * good.sum(), k
    s.close()


def test_two_identical_creates_give_bit_identical_taps(ctx, batches):
    b = batches["A"]
    for _ in range(2):
        s = _solver(ctx, b["problems"], b["draws"], b["min_set"], b["max_its"], b["reserve"])
        for k in range(len(b["problems"])):
            for tap, first in ((s.hypotheses(k), b["hyps"][k]), (s.refinements(k), b["refs"][k])):
                for key in ("count", "Rt", "inlier", "cws", "basis", "betas", "rep_error", "which"):
                    assert tap[key].tobytes() == first[key].tobytes(), (k, key)
        s.close()


def test_empty_and_single_batches(ctx, batches):
    e = _solver(ctx, [], np.zeros((0, 16, 4), "i4"), 4, 16, 0)
    e._ensure()
    assert _lib.load().ccm_pnp_solver_count(e._handle) == 0
    e.close()
    b = batches["A"]                                    # one solver alone gives the rows it gave inside the batch of 7
    s = _solver(ctx, b["problems"][4:5], b["draws"][4:5], b["min_set"], b["max_its"], b["reserve"])
    h = s.hypotheses(0)
    assert h["Rt"].tobytes() == b["hyps"][4]["Rt"].tobytes() and (h["count"] == b["hyps"][4]["count"]).all()
    assert s.refinements(0)["Rt"].tobytes() == b["refs"][4]["Rt"].tobytes()
    s.close()


def test_hundred_batches_reuse_the_context_pool(ctx, batches):
    import torch
    b = batches["A"]
    free1 = None
    for i in range(100):
        s = _solver(ctx, b["problems"], b["draws"], b["min_set"], b["max_its"], b["reserve"], detail=False)
        assert s.iterate(4, 5)[3] >= 0
        s.close()
        if i == 0:
            free1 = torch.cuda.mem_get_info()[0]
    assert torch.cuda.mem_get_info()[0] == free1


def _create(ctx, flat, draws, min_set=4, max_its=16, reserve=0, **over):
    a = dict(flat); a.update(over)
    p = _lib.ptr
    keep = [None if a[k] is None else np.ascontiguousarray(a[k]) for k in ("first", "n1", "K", "P2D", "P3Dw", "sigma2", "kp_index")]
    d = np.ascontiguousarray(draws, "i4")
    pb = _lib.PnpRansacProblem(len(a["n1"]), *[p(x) for x in keep], PROB, MIN_INLIERS, max_its, min_set, EPS, TH2, reserve, p(d), 0)
    h = C.c_void_p(0x5eed)
    rc = _lib.load().ccm_pnp_solver_create(ctx.handle, C.byref(pb), C.byref(h))
    return rc, h


def test_argument_errors_leave_the_outputs_untouched(ctx, batches):
    b = batches["A"]
    flat = ref.flatten(b["problems"][1:4]); d = b["draws"][1:4].copy()              # N = 4, 9, 63
    lib = _lib.load()
    rc, h = _create(ctx, flat, d)
    assert rc == 0 and h.value != 0x5eed
    assert lib.ccm_pnp_solver_hypotheses(h, 0, None, None, None, None, np.zeros(68).ctypes.data_as(C.c_void_p)) == -7      # no detail kept
    assert lib.ccm_pnp_solver_iterate(h, 3, 5, None, None, None, None, None) == -1      # no such solver
    found = C.c_int32(77)
    assert lib.ccm_pnp_solver_iterate(h, 0, 5, C.byref(found), None, None, None, None) == -1 and found.value == 77
    lib.ccm_pnp_solver_destroy(h)
    bad = d.copy(); bad[2, 7, 1] = 62                    # draw 1 of a solver with N = 63 must lie in [0, 61]
    first = flat["first"].copy(); first[1], first[2] = first[2], first[1]
    kp = flat["kp_index"].copy(); kp[3] = flat["n1"][0]
    for over, dd, kw, word in ((dict(), bad, {}, "draw"), (dict(P3Dw=None), d, {}, "null"), (dict(first=first), d, {}, "first"),
                               (dict(kp_index=kp), d, {}, "kp_index"), (dict(), d, dict(min_set=3), "min_set"), (dict(), d, dict(min_set=9), "min_set")):
        rc, h = _create(ctx, flat, dd, **kw, **over)
        assert rc == -1 and h.value == 0x5eed, word
        assert word in lib.ccm_last_error(ctx.handle).decode(), lib.ccm_last_error(ctx.handle)
    bad = d.copy(); bad[0, 0, 0] = -1
    assert _create(ctx, flat, bad)[0] == -1
    bad = d.copy(); bad[0, 12, 0] = 10 ** 6              # the solver with N = 4 evaluates one hypothesis: row 12 is never read
    rc, h = _create(ctx, flat, bad)
    assert rc == 0
    lib.ccm_pnp_solver_destroy(h)
    Rt = np.full(12, 7.0)
    assert lib.ccm_pnp_compute_pose(3, _lib.ptr(flat["P3Dw"]), _lib.ptr(flat["P2D"]), _lib.ptr(flat["K"]), _lib.ptr(Rt), None) == -1 and (Rt == 7.0).all()
