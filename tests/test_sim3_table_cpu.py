"""CPU-side checks of ccm_search_by_sim3_table_frames and ccm_search_by_projection_table_frames: the library exports them at ABI 3,
the ctypes mirror has the sizes and offsets a C compiler gives include/ccm_hot.h, known answers of the numpy restatement
tests/sim3_table_ref.py, and the conditions the scenes of the GPU tests must meet (with synthetic features in place of extracted ones)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fuse_table_ref as R
import search_local_points_ref as S
import sim3_table_ref as Q
from motioncheck_ccm_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ccm_search_by_sim3_table_frames", "ccm_search_by_projection_table_frames")
# the restatement numbers its gates as the header does (through the ctypes mirror)
assert [_lib.SG_GATES.index(n) for n in ("SEARCHED", "NO_POINT", "MATCHED", "BAD", "BEHIND", "OUTSIDE", "DISTANCE", "EMPTY_KF")] == [
    Q.SEARCHED, Q.NO_POINT, Q.MATCHED, Q.IS_BAD, Q.BEHIND, Q.OUTSIDE, Q.DISTANCE, Q.EMPTY_KF]
assert [_lib.LG_GATES.index(n) for n in ("SEARCHED", "SKIPPED", "ALREADY_FOUND", "BEHIND", "OUTSIDE", "DISTANCE", "ANGLE", "EMPTY_KF")] == [
    Q.LG_SEARCHED, Q.LG_SKIPPED, Q.LG_ALREADY_FOUND, Q.LG_BEHIND, Q.LG_OUTSIDE, Q.LG_DISTANCE, Q.LG_ANGLE, Q.LG_EMPTY_KF]
STRUCTS = (("ccm_sim3_search_pair", "Sim3SearchPair"), ("ccm_sim3_search_problem", "Sim3SearchProblem"), ("ccm_sim3_search_result", "Sim3SearchResult"),
           ("ccm_loop_view", "LoopView"), ("ccm_loop_projection_problem", "LoopProjectionProblem"), ("ccm_loop_projection_result", "LoopProjectionResult"))


def test_symbols_exist_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.ccm_abi_version() == 3 == _lib.ABI_VERSION
    txt = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ccm_hot.h")).read(), flags=re.S)
    assert "#define CCM_ABI_VERSION 3" in txt
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == 4 and re.search(r"\bint %s\(ccm_ctx\*, ccm_map_table\*, const \w+\*, \w+\*\);" % name, txt), name
    assert _lib.SG_GATES.index("EMPTY_KF") == 7 == _lib.LG_GATES.index("EMPTY_KF") and _lib.LG_GATES[2] == "ALREADY_FOUND"
    for k, n in enumerate(_lib.SG_GATES):
        assert re.search(r"CCM_SG_%s = %d\b" % (n, k), txt), n
    for k, n in enumerate(_lib.LG_GATES):
        assert re.search(r"CCM_LG_%s = %d\b" % (n, k), txt), n


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


def test_python_mirror_shim_and_documents_name_the_calls():
    from motioncheck_ccm_slam_amd.matcher import ORBmatcher
    assert callable(ORBmatcher.SearchBySim3TableFrames) and callable(ORBmatcher.SearchByProjectionTableFrames)
    shim = open(os.path.join(ROOT, "shim", "cslam_sim3solver.cpp")).read()
    for name in NAMES:
        assert name in shim, name
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in open(os.path.join(ROOT, doc)).read(), (doc, name)


def test_null_arguments_are_argument_errors():
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name)(None, None, None, None) == -1, name


# ---------------------------------------------------------------------------------------------------------------- known answers
def _shared_pair(s12=1.0, n=300, identity=False, seed=3):
    """kf1 and kf2 with a shared feature set under equal poses (the same dict twice)."""
    sc = Q.Sim3Scene(seed)
    kf = sc.keyframe(R.synthetic_features(n, seed), R.CAMERAS[0], frac=0.7)
    p = sc.pair(kf, n, None, s12, None, kf2=kf)
    if identity:
        I = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype("f4")
        p["S12"] = I; p["S21"] = I.copy()
    return sc.finish(), p


def test_identity_sim3_on_a_shared_feature_set_matches_every_feature_to_itself():
    scene, p = _shared_pair(identity=True)
    d1, d2 = Q.sim3_pair(scene, p)
    found, m12, sel1, sel2 = Q.sim3_select(p, d1, d2)
    valid = d1["gate"] == Q.SEARCHED
    assert valid.sum() >= 150 and (d1["gate"] == d2["gate"]).all()
    assert (m12[valid] == np.flatnonzero(valid)).all() and (m12[~valid] == -1).all() and found == valid.sum()
    # each point predicts its feature's own octave and lands within a pixel of it
    assert (d1["level"][valid] == p["kf1"]["oct"][valid]).all()
    assert np.abs(d1["u"][valid] - p["kf1"]["kx"][valid]).max() < 0.01


@pytest.mark.parametrize("s12", [2.0, 0.5])
def test_scale_shifts_the_predicted_level_and_distance_rejects_the_far_end(s12):
    scene, p = _shared_pair(s12=s12)
    p["S12"][:, 3] = 0; p["S21"][:, 3] = 0                       # pure scale and a small rotation: the distance changes by exactly s
    base, q = _shared_pair(identity=True)
    b1, _ = Q.sim3_pair(base, q)
    d1, d2 = Q.sim3_pair(scene, p)
    assert Q.SHIFT2 == 4
    oct1 = p["kf1"]["oct"]
    for d, sign in ((d1, +1 if s12 > 1 else -1), (d2, -1 if s12 > 1 else +1)):    # 1 -> 2 divides the distance by s12, 2 -> 1 multiplies it
        reached = np.isin(d["gate"], (Q.SEARCHED, Q.OUTSIDE, Q.DISTANCE)) & (b1["gate"] == Q.SEARCHED)
        far = d["gate"] == Q.DISTANCE
        ok = (d["gate"] == Q.SEARCHED) & (b1["gate"] == Q.SEARCHED)
        assert ok.sum() >= 10 and far.sum() >= 10 and reached.sum() >= ok.sum()
        want = np.clip(oct1 + sign * Q.SHIFT2, 0, Q.N_LEVELS - 1)
        assert (d["level"][ok] == want[ok]).all()
        if sign < 0:      # twice as far: max_dist = d 1.2^(o - 0.5) admits 2 d <= 1.2 max_dist only from octave 4 up
            assert (oct1[far & (b1["gate"] == Q.SEARCHED)] <= 3).all() and (oct1[ok] >= 4).all()
        else:             # half as far: 0.8 min_dist = 0.8 d 1.2^(o - 7.5) exceeds d / 2 from octave 5 up
            assert (oct1[far & (b1["gate"] == Q.SEARCHED)] >= 5).all() and (oct1[ok] <= 4).all()


def test_only_the_first_keyframes_intrinsics_are_used():
    scene, p = _shared_pair(identity=True)
    d1, d2 = Q.sim3_pair(scene, p)
    p2 = dict(p, intr2=(400.0, 410.0, 300.0, 200.0))             # pKF2 has a camera of its own: nothing reads it
    e1, e2 = Q.sim3_pair(scene, p2)
    for a, b in ((d1, e1), (d2, e2)):
        assert a["u"].tobytes() == b["u"].tobytes() and a["gate"].tobytes() == b["gate"].tobytes()
    p3 = dict(p, intr=p2["intr2"])                               # while pKF1's moves both directions
    f1, f2 = Q.sim3_pair(scene, p3)
    s = (d1["gate"] == Q.SEARCHED) & (f1["gate"] == Q.SEARCHED)
    assert s.sum() > 20 and (f1["u"][s] != d1["u"][s]).all() and (f2["u"][s] != d2["u"][s]).all()
    x = (d1["u"][s].astype("f8") - 367.0) / 458.0
    assert np.abs(f1["u"][s] - (400.0 * x + 300.0)).max() < 1e-2


def test_each_sim3_gate_in_the_reference_order():
    rows = S.matchable_points(np.array([300.0], "f4"), np.array([200.0], "f4"), np.array([2]), np.zeros((1, 32), np.uint8), *S.IDENTITY, seed=1)
    rows["flags"][:] = Q.LIVE
    I = S.IDENTITY[0]

    def one(ids=(0,), marked=(False,), flags=None, S21=I, bounds=Q.BOUNDS, n_target=5, mx=None):
        r = {k: v.copy() for k, v in rows.items()}
        if flags is not None:
            r["flags"][:] = flags
        if mx is not None:
            r["max_dist"][:] = mx
        return int(Q.sim3_direction(r, 1, ids, marked, I, S21, Q.INTR, bounds, n_target)["gate"][0])
    back = I.copy(); back[2, 2] = -1
    assert one() == Q.SEARCHED and one(n_target=0) == Q.EMPTY_KF
    assert one(ids=(-1,)) == one(ids=(1,)) == one(flags=0) == one(flags=Q.BAD) == Q.NO_POINT       # not LIVE comes before BAD
    assert one(marked=(True,), flags=Q.LIVE | Q.BAD) == Q.MATCHED and one(flags=Q.LIVE | Q.BAD, S21=back) == Q.IS_BAD
    assert one(S21=back, bounds=(0, 1, 0, 1)) == Q.BEHIND and one(bounds=(0, 299, 0, 480), mx=1e-3) == Q.OUTSIDE
    assert one(mx=1e-3, n_target=0) == Q.DISTANCE


def test_marks_ignore_indices_outside_the_second_keyframe():
    p = dict(kf2=dict(kx=np.zeros(4)), matched12=np.array([5, -1, 7, 8, 9, 3]), matched_idx2=np.array([1, 2, -1, 4, 9, 3]))
    a1, a2 = Q.marks(p)
    assert a1.tolist() == [True, False, True, True, True, True] and a2.tolist() == [False, True, False, True]


# ---------------------------------------------------------------------------------------------------------------- scene conditions
def test_sim3_scene_conditions():
    feat = R.synthetic_features(1000, 7)
    seen = np.zeros(8, int)
    n_amb = n_searched = 0
    for n1, n2, n_pairs in Q.SIM3_CASES:
        sc = Q.sim3_scene(feat, n1, n2, n_pairs)
        assert len(sc["pairs"]) == n_pairs and (n_pairs < 2 or sc["pairs"][0]["kf1"] is sc["pairs"][1]["kf1"])
        for p in sc["pairs"]:
            d1, d2 = Q.sim3_pair(sc, p)
            for d in (d1, d2):
                seen += np.bincount(d["gate"], minlength=8)
                n_amb += int(d["ambiguous"].sum()); n_searched += int((d["gate"] == Q.SEARCHED).sum())
            if min(n1, n2) >= 255:
                found, m12, _, _ = Q.sim3_select(p, d1, d2)
                assert found >= 5, (n1, n2, n_pairs, found)
    print("sim3 gates over the designed scenes: %s, ambiguous %d of %d" % (seen.tolist(), n_amb, n_searched))
    assert (seen >= 1).all() and n_amb <= 0.01 * n_searched
    assert {c[0] for c in Q.SIM3_CASES} == set(Q.SIM3_SIZES) == {c[1] for c in Q.SIM3_CASES} and {c[2] for c in Q.SIM3_CASES} == {1, 2, 3}


def test_loop_scene_conditions():
    feat = R.synthetic_features(1000, 7)
    seen = np.zeros(8, int)
    n_amb = n_searched = 0
    for n_points in (0, 1, 63, 64, 65, 257, 1025):
        for n_kf in (1, 2, 3):
            sc = Q.loop_scene(feat, n_points, n_kf)
            g = Q.loop_views(sc)
            if n_points:
                seen += np.bincount(g["gate"].ravel(), minlength=8)
                n_amb += int((g["ambiguous"] & (g["gate"] == Q.LG_SEARCHED)).sum()); n_searched += int((g["gate"] == Q.LG_SEARCHED).sum())
            nm, bi, ms = Q.loop_accept(sc, g)
            if n_points >= 255:
                assert (nm >= 5).all() and ((bi >= 0) & (g["observed"] == 1)).sum() >= 1, (n_points, n_kf, nm)
                assert (g["gate"] == Q.LG_ALREADY_FOUND).sum() >= n_kf
    empty = Q.loop_scene(feat, 65, 1, n_feat=0)
    seen += np.bincount(Q.loop_views(empty)["gate"].ravel(), minlength=8)
    print("loop gates over the designed scenes: %s, ambiguous %d of %d" % (seen.tolist(), n_amb, n_searched))
    assert (seen >= 1).all() and n_amb <= 0.01 * n_searched
    big = Q.big_loop_scene()
    g = Q.loop_views(big)
    nm, bi, _ = Q.loop_accept(big, g)
    assert nm[0] >= 100 and (g["ambiguous"] & (g["gate"] == Q.LG_SEARCHED)).sum() <= 0.01 * (g["gate"] == Q.LG_SEARCHED).sum()


def test_retry_scene_overflows_the_first_capacity_in_one_view_only():
    """What test_loop_projection_table_gpu.py's capacity-retry case relies on, from the definition alone: the crowded view's lists are
    longer than the device route's first capacity of 64, the sparse view's are not, and the sparse view accepts a match (so the first
    attempt has written flags and a choice there before every view repeats)."""
    sc = Q.retry_scene()
    sparse, crowded = Q.longest_lists(sc)
    assert crowded >= 65 and 1 <= sparse <= 64, (sparse, crowded)
    nm, bi, ms = Q.loop_accept(sc, Q.loop_views(sc))
    assert nm[0] >= 1 and bi[0].tolist() == [0, -1] and bi[1].tolist() == [37, -1] and ms[1][37] == 0


def test_hand_built_order_cases_of_the_restatement():
    # two points whose windows share their nearest feature: the first in the list takes it, the second its next best
    sc = Q.hand_scene(*Q.HAND_SHARED)
    nm, bi, ms = Q.loop_accept(sc, Q.loop_views(sc))
    assert bi[0].tolist() == [0, -1] and nm[0] == 1 and ms[0].tolist() == [0, -1]      # distances 2 | 49 and 1 | 52: the second gets nothing
    sc = Q.hand_scene(Q.HAND_SHARED[0], Q.HAND_SHARED[1][::-1])
    nm, bi, ms = Q.loop_accept(sc, Q.loop_views(sc))
    assert bi[0].tolist() == [0, 1] and nm[0] == 2 and ms[0].tolist() == [0, 1]        # swapped: the other point owns feature 0, this one takes its next best
    # exactly TH_LOW is accepted, one more is not
    sc = Q.hand_scene([(300.0, 200.0, 2, 0), (500.0, 300.0, 2, 0)], [(300.0, 200.0, 2, 50), (500.0, 300.0, 2, 51)])
    nm, bi, _ = Q.loop_accept(sc, Q.loop_views(sc))
    assert bi[0].tolist() == [0, -1] and nm[0] == 1
