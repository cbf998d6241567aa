"""CPU-side checks of ccm_sim3_solver_create_frames, ccm_optimize_sim3_table_frames and ccm_compute_sim3_table_frames: the library
exports them at ABI 3, the ctypes mirror has the sizes and offsets a C compiler gives include/ccm_hot.h, NULL arguments are refused
before a device is touched, known answers of the restatement's correspondence filter (tests/compute_sim3_ref.py), the conditions the
scenes of test_compute_sim3_gpu.py must meet -- shown by the restated chain and the CPU oracle's OptimizeSim3 -- and the pass logic
of loopclosing.ComputeSim3 against the sequential loop of the reference with stubbed solvers and chain results."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import compute_sim3_ref as X
import sim3_solver_ref as SR
from motioncheck_ccm_slam_amd import _lib, loopclosing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ccm_sim3_solver_create_frames", "ccm_optimize_sim3_table_frames", "ccm_compute_sim3_table_frames")
STRUCTS = (("ccm_sim3_frames_pair", "Sim3FramesPair"), ("ccm_sim3_solver_frames_problem", "Sim3SolverFramesProblem"),
           ("ccm_sim3_opt_frames_problem", "Sim3OptFramesProblem"), ("ccm_sim3_opt_frames_result", "Sim3OptFramesResult"),
           ("ccm_compute_sim3_pair", "ComputeSim3Pair"), ("ccm_compute_sim3_problem", "ComputeSim3Problem"), ("ccm_compute_sim3_result", "ComputeSim3Result"))


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ccm_abi_version() == 3 == _lib.ABI_VERSION
    txt = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ccm_hot.h")).read(), flags=re.S)
    assert "#define CCM_ABI_VERSION 3" in txt
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == 4 and re.search(r"\bint %s\(ccm_ctx\*, ccm_map_table\*, const \w+\*, [\w*]+( out)?\);" % name, txt), name


def test_structures_have_the_compilers_sizes_and_offsets(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no host compiler")
    lines = []
    for cname, pname in STRUCTS:
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for f, _ in getattr(_lib, pname)._fields_:
            lines.append('printf(" %%zu", offsetof(%s, %s));' % (cname, f))
        lines.append('printf("\\n");')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccm_hot.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.stdout.splitlines()}
    for cname, pname in STRUCTS:
        T = getattr(_lib, pname)
        assert got[cname] == [C.sizeof(T)] + [getattr(T, f).offset for f, _ in T._fields_], cname


def test_null_arguments_are_argument_errors():
    lib = _lib.load()
    out = C.c_void_p(123)
    assert lib.ccm_sim3_solver_create_frames(None, None, None, C.byref(out)) == -1 and out.value == 123
    for name in NAMES:
        assert getattr(lib, name)(None, None, None, None) == -1, name


def test_python_mirror_shim_and_documents_name_the_calls():
    from motioncheck_ccm_slam_amd.matcher import ORBmatcher
    from motioncheck_ccm_slam_amd.optimizer import Optimizer
    from motioncheck_ccm_slam_amd.sim3solver import Sim3Solver
    assert callable(ORBmatcher.ComputeSim3TableFrames) and callable(Optimizer.OptimizeSim3TableFrames) and callable(Sim3Solver.from_frames)
    assert callable(loopclosing.ComputeSim3)
    shim = open(os.path.join(ROOT, "shim", "cslam_sim3solver.cpp")).read()
    for name in NAMES:
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (doc, name)
    assert "ccm_sim3_solver_create_frames" in shim and "ccm_compute_sim3_table_frames" in shim
    assert "sim3_solvers_on_table" in shim and "compute_sim3_candidates_on_table" in shim


def test_max_err_level_drops_the_fraction_as_a_size_t_vector_does():
    from motioncheck_ccm_slam_amd.sim3solver import level_max_err
    assert X.MAX_ERR_LEVEL.tolist() == [9.0, 13.0, 19.0, 27.0, 39.0, 57.0, 82.0, 118.0]
    assert level_max_err(X.LEVEL_SIGMA2).tobytes() == X.MAX_ERR_LEVEL.tobytes()


# ---------------------------------------------------------------------------------------------------------------- known answers
def test_the_correspondence_filter_of_optimize_sim3():
    """Six features on side 1, four on side 2, slots 0..7 of a table of capacity 8: slot 5 is BAD, slot 6 not LIVE."""
    flags = np.array([1, 1, 1, 1, 1, 3, 0, 1], np.uint8)
    kf1 = dict(kx=np.zeros(6), mp_id=np.array([0, 1, 5, 6, -1, 2], "i4"))
    kf2 = dict(kx=np.zeros(4), mp_id=np.array([3, 4, 5, 7], "i4"))
    rows = dict(flags=flags)

    def run(m12_in, mi2, match12):
        p = dict(kf1=kf1, kf2=kf2, matched12=np.array(m12_in, "i4"), matched_idx2=np.array(mi2, "i4"))
        return X.correspondences(rows, 8, p, np.array(match12, "i4")).tolist()
    none = [-1] * 6
    assert run(none, none, none) == []
    assert run(none, none, [0, 1, -1, -1, -1, 3]) == [[0, 0], [1, 1], [5, 3]]              # SearchBySim3's matches, ascending i1
    assert run([9, -1, -1, -1, -1, -1], [3, -1, -1, -1, -1, -1], [1, 0, -1, -1, -1, -1]) == [[0, 3], [1, 0]]   # the solver's inlier wins over match12
    assert run([9, 9, 9, -1, -1, -1], [-1, 4, 2, -1, -1, -1], none) == []                  # no index in kf2, one past it, a BAD point on side 2
    assert run(none, none, [-1, -1, 0, 0, 0, -1]) == []                                     # side 1: BAD, not LIVE, no point
    assert run([9, -1, -1, -1, -1, -1], [0, -1, -1, -1, -1, -1], [-1, 0, -1, -1, -1, -1]) == [[0, 0], [1, 0]]  # two features may name one i2


def test_gathered_arrays_are_the_matrix_product_and_the_level_tables():
    sc = X.gather_scene(90, 80, seed=3)
    p = sc["pairs"][0]
    c = X.pick_correspondences(sc, p, 12, np.random.default_rng(0))
    a = X.solver_arrays(sc["rows"], p, c[:, 0], c[:, 1]); o = X.opt_arrays(sc["rows"], p, c[:, 0], c[:, 1])
    s1, s2 = X.slots(p, c[:, 0], c[:, 1])
    T1 = np.asarray(p["T1w"], "f8")
    want = sc["rows"]["pos"][s1].astype("f8") @ T1[:, :3].T + T1[:, 3]
    assert np.abs(a["X1"] - want).max() < 1e-5 and a["X1"].dtype == np.float32 and (o["P1"] == a["X1"].astype("f8")).all()
    assert (a["max_err1"] == X.MAX_ERR_LEVEL[p["kf1"]["oct"][c[:, 0]]]).all() and (o["info2"] == X.INV_SIGMA2[p["kf2"]["oct"][c[:, 1]]].astype("f8")).all()
    assert (o["obs2"][:, 0] == p["kf2"]["kx"][c[:, 1]].astype("f8")).all() and (np.diff(c[:, 0]) > 0).all()


# ---------------------------------------------------------------------------------------------------------------- scene conditions
def test_gather_scenes_hold_enough_live_correspondences():
    sc = X.gather_scene(90, 80, seed=3)
    p = sc["pairs"][0]
    assert len(X.live_features(sc, p["kf1"])) >= max(X.SOLVER_SIZES) and len(X.true_pairs(sc, p)) >= 12
    rng = np.random.default_rng(1)
    for n in X.SOLVER_SIZES:
        c = X.pick_correspondences(sc, p, n, rng)
        assert len(c) == n and len(set(c[:, 0].tolist())) == n
    fl = sc["rows"]["flags"]
    assert any((fl[p["kf1"]["mp_id"][i]] & X.BAD) for i in X.live_features(sc, p["kf1"]))     # a BAD slot among them: accepted
    big = X.gather_scene(600, 600, seed=4)
    assert len(X.true_pairs(big, big["pairs"][0])) >= 200 and len(X.live_features(big, big["pairs"][0]["kf1"])) >= max(X.OPT_SIZES)


def test_chain_scene_conditions(oracle):
    sc = X.chain_scene()
    assert [len(p["kf1"]["kx"]) for p in sc["pairs"]] == list(X.CHAIN_N1)
    assert sc["pairs"][2]["kf1"] is sc["pairs"][2]["kf2"] and tuple(sc["pairs"][3]["intr2"]) != tuple(sc["pairs"][3]["intr"])
    res = []
    left_bad = 0
    for p in sc["pairs"]:
        found, m12 = X.search_pair(sc, p)
        r = X.chain_pair(sc, p, m12, oracle.optimize_sim3)
        r["survivors"] = len(r["corr"]) - int(r["pruned"].sum())
        res.append(r)
        if "bad_i1" in p:
            i1 = p["bad_i1"]
            assert p["matched12"][i1] >= 0 and 0 <= p["matched_idx2"][i1] < len(p["kf2"]["kx"]) and i1 not in r["corr"][:, 0] and r["pruned"][i1] == 0
            left_bad += 1
        if r["n_inliers"] == 0:
            assert (r["sim3"] == np.asarray(p["sim3"])).all()
        print("n1 = %d: found %d, correspondences %d, pruned %d, n_inliers %d" % (len(p["kf1"]["kx"]), found, len(r["corr"]), r["pruned"].sum(), r["n_inliers"]))
    assert any(r["n_inliers"] >= 20 for r in res)                                           # a pair accepted
    assert any(1 <= r["survivors"] <= 9 for r in res)                                       # a pair below the ten-survivor rule
    assert any(r["pruned"].any() for r in res) and left_bad >= 1
    assert len(res[0]["corr"]) == 0 and res[0]["n_inliers"] == 0


# ---------------------------------------------------------------------------------------------------------------- the driver's passes
class _StubSolvers:
    """n RefSolvers behind the interface loopclosing.ComputeSim3 reads: hypothesis h of solver k 'returns a Sim3' named (k, h)."""

    def __init__(self, counts, n=30, min_inliers=6):
        self.k = [SR.RefSolver(n, n, np.arange(n), c, np.arange(n)[None, :] < np.asarray(c)[:, None], min_inliers, len(c)) for c in counts]
        self.n = len(self.k)
        self.last = [None] * self.n

    def iterate(self, k, its):
        h, no_more, vb, nin = self.k[k].iterate(its)
        self.last[k] = h
        return (None if h is None else np.full((4, 4), 100 * k + h, "f4")), no_more, vb, nin

    def GetEstimatedRotation(self, k):
        return ("R", k, self.k[k].best)

    def GetEstimatedTranslation(self, k):
        return ("t", k, self.k[k].best)

    def GetEstimatedScale(self, k):
        return ("s", k, self.k[k].best)


class _One:
    """Solver k of a _StubSolvers as the sequential restatement reads it."""

    def __init__(self, solvers, k):
        self.solvers, self.k = solvers, k

    def iterate(self, its):
        return self.solvers.iterate(self.k, its)


@pytest.mark.parametrize("seed", range(12))
def test_compute_sim3_passes_return_what_the_sequential_loop_returns(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 5))
    counts = [rng.integers(0, 12, int(rng.integers(3, 40))) for _ in range(n)]
    verdict = {(k, h): int(rng.choice([0, 5, 19, 20, 45], p=[0.3, 0.3, 0.2, 0.1, 0.1])) for k in range(n) for h in range(len(counts[k]))}
    if seed % 4 == 3:
        verdict = {key: min(v, 19) for key, v in verdict.items()}                           # nobody matches: every solver runs dry
    seq = _StubSolvers(counts)
    want, _ = X.compute_sim3_sequential([_One(seq, k) for k in range(n)], lambda i, Scm, vb: dict(n_inliers=verdict[(i, seq.last[i])], h=seq.last[i]))
    par = _StubSolvers(counts)
    batches = []

    def chain(items):
        batches.append([it[0] for it in items])
        assert all(it[2] == ("R", it[0], par.last[it[0]]) for it in items)                  # the estimate of the hypothesis that came back
        return [dict(n_inliers=verdict[(it[0], par.last[it[0]])], h=par.last[it[0]]) for it in items]
    got = loopclosing.ComputeSim3(par, chain)
    if want is None:
        assert got is None
        assert all(s.mnIterations == t.mnIterations for s, t in zip(seq.k, par.k))          # identical solver state when nobody matches
    else:
        i, res, vb = want
        assert got["candidate"] == i and got["h"] == res["h"] and got["n_inliers"] == res["n_inliers"] and (got["inliers"] == vb).all()
    assert all(b == sorted(b) and len(b) >= 1 for b in batches)                             # one call per pass, candidates in order
