"""HIP bundle adjustment on the cases of tests/ba_cases.py: small graphs that sit on the size rules of the BA kernels (solver
switches, list lengths, inactive edges).  One iteration is held to the float64 numpy definition ba_cases.one_step, which owes nothing
to the oracle; whole schedules are held to the CPU oracle, within bounds derived from the oracle's own sensitivity
(ba_cases.SENS, measured by tests/test_ba_cases_cpu.py); schur_pairs / schur_blocks are held to a count made outside the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ba_cases as B
from motioncheck_ccm_slam_amd import optimizer
from motioncheck_ccm_slam_amd.optimizer import Optimizer, pose_delta

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)

_REF = {}


def _ref(oracle, name, label):
    """The oracle on a case (once per session), with its block-sparse solver: the same result as the dense one within the case's
    sensitivity, which test_ba_cases_cpu.py holds, and a hundred times sooner at 257 keyframes."""
    if (name, label) not in _REF:
        its, huber, its2 = {s[0]: s[1:] for s in B.SCHEDULES}[label]
        try:
            oracle.ba_set_solver(2)
            _REF[name, label] = oracle.ba_solve(B.case(name), its, huber, its2)
        finally:
            oracle.ba_set_solver(0)
    return _REF[name, label]


def _run(ctx, g, label, pcg_tol=0.0):
    if pcg_tol == 0.0:
        return Optimizer.BundleAdjustmentClient(g, 3, ctx=ctx) if label == "global3" else Optimizer.LocalBundleAdjustmentClient(g, ctx=ctx)
    its, huber, its2 = {s[0]: s[1:] for s in B.SCHEDULES}[label]
    return optimizer._solve(ctx, g, its, huber, its2, None, pcg_tol, want_outliers=its2 > 0)


def _check_structure(g, r):
    assert dict(schur_pairs=r["schur_pairs"], schur_blocks=r["schur_blocks"]) == B.structure_counts(g)
    fx = g["fixed"] != 0
    assert (r["poses"][fx] == g["poses"][fx]).all()                                    # fixed keyframes: not a bit changes


def _check_against_oracle(name, g, r, ref, pose_tol, point_tol, label, lam_tol=None, contract=False):
    """contract: the pose figure is pose_delta (|log(T T_ref^-1)| per keyframe, the contract of test_ba_gpu.py) instead of the largest
    change of an entry of R and of t."""
    R, t = B.pose_Rt(r["poses"]); Rr, tr = B.pose_Rt(ref["poses"])
    d = (float(np.abs(R - Rr).max()), float(np.abs(t - tr).max()), float(np.abs(r["points"] - ref["points"]).max()))
    if contract:
        d = (float(pose_delta(r["poses"], ref["poses"]).max()), 0.0, d[2])
    lam = abs(r["lambda_final"] / ref["lambda_final"] - 1.0)
    lam_tol = B.bound(B.SENS[name][3], B.LAMBDA_CAP) if lam_tol is None else lam_tol
    print("%-15s %-7s |dR| %.2e |dt| %.2e (bound %.2e) |dX| %.2e (bound %.2e) lambda %.2e (bound %.2e) pcg %d" %
          ((name, label) + d[:2] + (pose_tol, d[2], point_tol, lam, lam_tol, r["pcg_iterations"])))
    assert r["iterations_done"] == ref["iterations_done"] and r["trials"] == ref["trials"], (r["iterations_done"], r["trials"])
    if r["outlier"] is not None:
        assert (r["outlier"] == ref["outlier"]).all()
    assert max(d[:2]) <= pose_tol and d[2] <= point_tol, d
    assert np.isclose(r["chi2_initial"], ref["chi2_initial"], rtol=B.CHI2_INITIAL_RTOL, atol=0)
    assert np.isclose(r["chi2_final"], ref["chi2_final"], rtol=B.CHI2_RTOL, atol=0)
    assert lam <= lam_tol, lam


@pytest.mark.parametrize("robust", [True, False])
@pytest.mark.parametrize("name", B.ONE_STEP_CASES)
def test_one_iteration_is_the_numpy_definition(ctx, name, robust):
    """BundleAdjustmentClient(g, 1) against one_step: poses, points, the trials of the iteration and the lambda it leaves."""
    g = B.case(name)
    a = B.one_step(g, B.HUBER_GLOBAL if robust else 0.0)
    r = Optimizer.BundleAdjustmentClient(g, 1, bRobust=robust, ctx=ctx)
    R, t = B.pose_Rt(r["poses"])
    tol = B.bound(B.SENS[name][0], B.DENSE_POINT_CAP)
    d = (float(np.abs(R - a["R"]).max()), float(np.abs(t - a["t"]).max()), float(np.abs(r["points"] - a["points"]).max()))
    lam = abs(r["lambda_final"] / a["lam_final"] - 1.0)
    print("%-15s robust %d: |dR| %.2e |dt| %.2e |dX| %.2e (bound %.2e), lambda %.2e, %d trials" % ((name, robust) + d + (tol, lam, r["trials"])))
    assert r["iterations_done"] == 1 and r["trials"] == a["trials"] and r["pcg_iterations"] == 0
    assert max(d) <= tol, d
    assert lam <= B.bound(B.SENS[name][3], B.LAMBDA_CAP), lam
    _check_structure(g, r)


@pytest.mark.parametrize("name", B.FULL_CASES)
def test_full_schedules_against_the_oracle(ctx, oracle, name):
    """BundleAdjustmentClient(g, 3) and LocalBundleAdjustmentClient(g) under the default environment: the small dense solve up to 23
    free keyframes, the blocked inverse up to 256, the PCG (pipelined, coarse level on) at 257, there also at pcg_tol 1e-13 (classic
    iteration, held to the bound derived from the oracle's sensitivity)."""
    g = B.case(name)
    ru = B.rules(g)
    missed = []
    for k, (label, *_rest) in enumerate(B.SCHEDULES):
        ref = _ref(oracle, name, label)
        r = _run(ctx, g, label)
        _check_structure(g, r)
        if ru["pcg"]:
            assert r["pcg_iterations"] > 0 and r["pcg_fallbacks"] == 0 and r["pcg_pipelined"] == 1
            strict = _run(ctx, g, label, 1e-13)
            assert strict["pcg_iterations"] > 0 and strict["pcg_fallbacks"] == 0 and strict["pcg_pipelined"] == 0
            _check_structure(g, strict)
            tol = B.bound(B.SENS[name][1 + k], B.PCG_EXACT_CAP)
            for args in ((r, B.PCG_DEFAULT_POSE, B.PCG_DEFAULT_POINT, label, B.LAMBDA_CAP, True),        # inexact by design: the contract
                         (strict, tol, tol, label + "*", None, False)):
                try:                                                                             # (every figure is printed before the test fails)
                    _check_against_oracle(name, g, args[0], ref, *args[1:])
                except AssertionError as e:
                    missed.append("%s: %s" % (args[3], str(e).splitlines()[0]))
        else:
            assert r["pcg_iterations"] == 0
            s = B.SENS[name][1 + k]
            _check_against_oracle(name, g, r, ref, B.bound(s, B.DENSE_POSE_CAP), B.bound(s, B.DENSE_POINT_CAP), label)
        if name in B.S_CASES and label == "local":
            kf = B.stranded_keyframe(ru["nfree"])
            tol = B.bound(B.SENS[name][1 + k], B.DENSE_POINT_CAP)
            assert r["outlier"][g["moved"]].all()
            assert np.abs(r["poses"][kf] - ref["poses"][kf]).max() <= tol and np.abs(r["points"][0] - ref["points"][0]).max() <= tol
    assert not missed, missed


def _same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("poses", "points", "outlier")) and \
        (a["chi2_final"], a["lambda_final"], a["trials"]) == (b["chi2_final"], b["lambda_final"], b["trials"])


@pytest.mark.parametrize("name", ["L60", "S10", "S30"])
def test_a_second_call_and_a_shuffled_edge_list_give_the_same_bytes(ctx, name):
    g = B.case(name)
    r = Optimizer.LocalBundleAdjustmentClient(g, ctx=ctx)
    assert _same_bytes(r, Optimizer.LocalBundleAdjustmentClient(g, ctx=ctx))
    if name == "L60":
        o = np.random.default_rng(5).permutation(len(g["edge_pose"]))
        r2 = Optimizer.LocalBundleAdjustmentClient(B.reordered(g, o), ctx=ctx)
        assert r["outlier"].sum() > 0 and _same_bytes(dict(r, outlier=r["outlier"][o]), r2)
        assert (r2["schur_pairs"], r2["schur_blocks"]) == (r["schur_pairs"], r["schur_blocks"])


# ------------------------------------------------------------------------------------------------------------ child processes
# (the BA reads its environment once per process)
_CHILD_ENV = dict(PYTHONPATH=os.pathsep.join([ROOT, TESTS]))

_PCG_CHILD = r'''
import hashlib, sys
import numpy as np
import ba_cases as B
from motioncheck_ccm_slam_amd import _lib, optimizer
from motioncheck_ccm_slam_amd.optimizer import pose_delta
from oracle import oracle_py as O
ctx = _lib.Context(0)
O.ba_set_solver(2)
for name, (k, (label, its, huber, its2)) in ((n, s) for n in sys.argv[1:] for s in enumerate(B.SCHEDULES)):
    g = B.case(name)
    ref = O.ba_solve(g, its, huber, its2)
    for pcg_tol in (0.0, 1e-13):
        r = optimizer._solve(ctx, g, its, huber, its2, None, pcg_tol, want_outliers=its2 > 0)
        R, t = B.pose_Rt(r["poses"]); Rr, tr = B.pose_Rt(ref["poses"])
        d = (float(np.abs(R - Rr).max()), float(np.abs(t - tr).max()), float(np.abs(r["points"] - ref["points"]).max()))
        exact = B.bound(B.SENS[name][1 + k], B.PCG_EXACT_CAP)
        pose_tol, point_tol = (B.PCG_DEFAULT_POSE, B.PCG_DEFAULT_POINT) if pcg_tol == 0.0 else (exact, exact)
        lam = abs(r["lambda_final"] / ref["lambda_final"] - 1.0)
        print("%-5s %-7s pcg_tol %-6g |dR| %.2e |dt| %.2e |dX| %.2e (bounds %.2e %.2e) lambda %.2e, %d PCG iterations" %
              ((name, label, pcg_tol) + d + (pose_tol, point_tol, lam, r["pcg_iterations"])), flush=True)
        if pcg_tol == 0.0:
            d = (float(pose_delta(r["poses"], ref["poses"]).max()), 0.0, d[2])              # the contract's pose figure
        checks = {
            "PCG ran without fallback": r["pcg_iterations"] > 0 and r["pcg_fallbacks"] == 0,
            "pipelined as requested": r["pcg_pipelined"] == (1 if pcg_tol == 0.0 else 0),
            "structure counts": dict(schur_pairs=r["schur_pairs"], schur_blocks=r["schur_blocks"]) == B.structure_counts(g),
            "fixed keyframes": bool((r["poses"][g["fixed"] != 0] == g["poses"][g["fixed"] != 0]).all()),
            "iterations and trials": r["iterations_done"] == ref["iterations_done"] and r["trials"] == ref["trials"],
            "outlier flags": not its2 or bool((r["outlier"] == ref["outlier"]).all()),
            "poses and points": max(d[:2]) <= pose_tol and d[2] <= point_tol,
            "chi2": bool(np.isclose(r["chi2_initial"], ref["chi2_initial"], rtol=B.CHI2_INITIAL_RTOL, atol=0) and
                         np.isclose(r["chi2_final"], ref["chi2_final"], rtol=B.CHI2_RTOL, atol=0)),
            "lambda_final": lam <= (B.bound(B.SENS[name][3], B.LAMBDA_CAP) if pcg_tol else B.LAMBDA_CAP),
        }
        digest = hashlib.sha1(np.ascontiguousarray(r["poses"]).tobytes() + np.ascontiguousarray(r["points"]).tobytes()).hexdigest()
        print("RESULT %s %s %g %s %d %s" % (name, label, pcg_tol, ";".join(w.replace(" ", "_") for w, good in checks.items() if not good) or "ok",
                                           r["pcg_iterations"], digest), flush=True)
        print("    fallbacks %d, pipelined %d, trials %d / %d, chi2 %.12g / %.12g" %
              (r["pcg_fallbacks"], r["pcg_pipelined"], r["trials"], ref["trials"], r["chi2_final"], ref["chi2_final"]), flush=True)
ctx.close()
print("done")
'''

PCG_CASES = tuple(B.P_CASES) + ("S30",)
COARSE_CASES = ("P144", "P145")


def _pcg_child(cases, **extra):
    env = dict(os.environ, CCM_BA_DENSE_MAX="0", **_CHILD_ENV, **extra)
    out = subprocess.run([sys.executable, "-c", _PCG_CHILD] + list(cases), env=env, capture_output=True, text=True, timeout=300)
    print(out.stdout[-12000:])
    assert out.returncode == 0 and out.stdout.strip().endswith("done"), out.stdout[-3000:] + out.stderr[-3000:]
    report = {}
    for line in out.stdout.splitlines():
        if line.startswith("RESULT "):
            _, name, label, tol, verdict, its, digest = line.split()
            report[name, label, float(tol)] = (verdict, int(its), digest)
    return report


@pytest.fixture(scope="module")
def forced_pcg():
    """One child process with CCM_BA_DENSE_MAX=0 runs every forced-PCG case; its report per (case, schedule, pcg_tol): the verdict
    of the checks against the oracle, the PCG iterations, a digest of poses and points."""
    return _pcg_child(PCG_CASES)


@pytest.fixture(scope="module")
def forced_pcg_cluster_level_alone():
    """The same child with CCM_PCG_COARSE=0 (the cluster level alone) on the two graphs either side of nc >= 64."""
    return _pcg_child(COARSE_CASES, CCM_PCG_COARSE="0")


@pytest.mark.parametrize("pcg_tol", [0.0, 1e-13])
@pytest.mark.parametrize("label", [s[0] for s in B.SCHEDULES])
@pytest.mark.parametrize("name", PCG_CASES)
def test_forced_pcg_on_cluster_block_and_coarse_remainders(forced_pcg, name, label, pcg_tol):
    """CCM_BA_DENSE_MAX=0 sends every graph through the PCG: 1, 7, 8, 9 free keyframes around the 8-keyframe cluster, 17, 31, 32, 33
    around the 32-keyframe update block, 144 (63 coarse unknowns: coarse level off), 145 (70: on, pitch 96) and 161, and the
    inactive-edge graph S30, both schedules, each at the default pcg_tol (pipelined iteration) and at 1e-13 (classic iteration).
    Against the oracle: the bound derived from its sensitivity (at most 1e-9) at 1e-13, the contract of test_ba_gpu.py (pose_delta
    and points 1e-5, chi2 1e-9, lambda 1e-6) at the default tolerance."""
    verdict = forced_pcg[name, label, pcg_tol][0]
    assert verdict == "ok", verdict


@pytest.mark.parametrize("pcg_tol", [0.0, 1e-13])
@pytest.mark.parametrize("label", [s[0] for s in B.SCHEDULES])
def test_coarse_level_starts_at_145_free_keyframes(forced_pcg, forced_pcg_cluster_level_alone, label, pcg_tol):
    """The second preconditioner level is on from 64 coarse unknowns: 144 free keyframes (nc = 63) must not notice CCM_PCG_COARSE=0
    -- the same bytes after the same PCG iterations -- and 145 (nc = 70) must: other iteration counts, other bytes, and still the
    oracle's result."""
    alone = forced_pcg_cluster_level_alone
    assert alone["P144", label, pcg_tol] == forced_pcg["P144", label, pcg_tol]
    v0, its0, digest0 = forced_pcg["P145", label, pcg_tol]
    v1, its1, digest1 = alone["P145", label, pcg_tol]
    print("P145 %s pcg_tol %g: %d PCG iterations with the coarse level, %d without" % (label, pcg_tol, its0, its1))
    assert v1 == "ok" and alone["P144", label, pcg_tol][0] == "ok"
    assert its0 != its1 and digest0 != digest1


_REJECT_CHILD = r'''
import hashlib
import numpy as np
import ba_cases as B
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.optimizer import Optimizer
ctx = _lib.Context(0)
g = B.case("L60")
for r in (Optimizer.BundleAdjustmentClient(g, 6, ctx=ctx), Optimizer.LocalBundleAdjustmentClient(g, ctx=ctx)):
    assert r["trials"] > r["iterations_done"], (r["trials"], r["iterations_done"])
    assert r["chi2_final"] < 0.2 * r["chi2_initial"]
    print(hashlib.sha1(np.ascontiguousarray(r["poses"]).tobytes() + np.ascontiguousarray(r["points"]).tobytes()).hexdigest(), r["trials"])
ctx.close()
'''


def test_rejected_trial_on_long_observation_lists():
    """The L graph (lists of up to 60 free edges) with the first trial of iteration 2 rejected by the test switch: the run must
    repeat bit for bit what a build that always keeps Hpl computes, and what a run without the look-ahead computes."""
    procs = []
    try:
        for extra in ({}, {"CCM_BA_KEEP_HPL": "1"}, {"CCM_BA_NO_LOOKAHEAD": "1"}):
            env = dict(os.environ, CCM_BA_TEST_REJECT_AT="2", **_CHILD_ENV, **extra)
            procs.append(subprocess.Popen([sys.executable, "-c", _REJECT_CHILD], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        outs = [p.communicate(timeout=300) + (p.returncode,) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for o, e, rc in outs:
        assert rc == 0, o[-2000:] + e[-2000:]
    lines = [o.split() for o, _, _ in outs]
    assert len(lines[0]) == 4 and lines[0] == lines[1] == lines[2], lines
