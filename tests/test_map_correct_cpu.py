"""ccm_map_table_correct_frames (include/ccm_hot.h "loop and merge corrections on the table") on the CPU: declared, exported, mirrored
field for field, refusing NULL arguments before it touches a device; known answers of the numpy restatement
tests/map_correct_ref.py that the GPU tests compare against, and the condition its scene must fulfil so that the GPU test of the
order rule cannot pass trivially.  No GPU work here."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import map_correct_ref as MC
import map_refresh_ref as R
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.optimizer import pose_to_camera
from optimizer_cases import correct_map_points_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


def _rows(C_):
    return {k: v[C_["S"]["slot"]] for k, v in R.table_rows(2).items()}


def test_entry_point_declared_exported_and_mirrored():
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ccm_hot.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ccm_map_table_correct_frames\s*\(\s*ccm_ctx\s*\*\s*,\s*ccm_map_table\s*\*\s*,\s*const\s+ccm_map_correct\s*\*\s*\)\s*;", h)
    body = re.search(r"typedef\s+struct\s*{([^}]*)}\s*ccm_map_correct\s*;", h).group(1)
    declared = [re.search(r"(\w+)\s*$", d).group(1) for st in body.split(";") if st.strip() for d in st.split(",")]
    assert declared == [f[0] for f in _lib.MapCorrect._fields_], declared
    assert declared == ["n_kf", "kfs", "n_moved", "transform", "order", "sim3_before", "sim3_after", "Tcw_after", "Ow_after", "n_points", "slot",
                        "owner", "obs_first", "obs_kf", "obs_feat", "ref_kf", "ref_feat", "pos_out", "normal_out", "min_dist_out", "max_dist_out"]
    ints = {"n_kf", "n_moved", "transform", "order", "n_points"}
    for name, typ in _lib.MapCorrect._fields_:
        assert (typ is C.c_int32) == (name in ints), name
    assert re.search(r"\bCCM_MC_SIM3\s*=\s*0\b", h) and re.search(r"\bCCM_MC_RIGID\s*=\s*1\b", h)
    assert re.search(r"\bCCM_MC_POSES_FIRST\s*=\s*0\b", h) and re.search(r"\bCCM_MC_IN_ORDER\s*=\s*1\b", h)
    assert (_lib.MC_SIM3, _lib.MC_RIGID) == (MC.SIM3, MC.RIGID) == (0, 1)
    assert (_lib.MC_POSES_FIRST, _lib.MC_IN_ORDER) == (MC.POSES_FIRST, MC.IN_ORDER) == (0, 1)
    lib = _lib.load()
    assert "ccm_map_table_correct_frames" in _lib.SYMBOLS and hasattr(lib, "ccm_map_table_correct_frames")
    assert lib.ccm_abi_version() == 3 == _lib.ABI_VERSION         # additions only


def test_null_context_table_or_problem_is_an_argument_error():
    lib = _lib.load()
    slot = np.zeros(1, "i4"); owner = np.full(1, -1, "i4"); pos = np.full((1, 3), 77, "f4")
    u = _lib.MapCorrect(0, None, 0, 0, 0, None, None, None, None, 1, _lib.ptr(slot), _lib.ptr(owner), None, None, None, None, None,
                        _lib.ptr(pos), None, None, None)
    fake = C.c_void_p(8)                                          # never dereferenced: the NULL argument is found first
    assert lib.ccm_map_table_correct_frames(None, None, C.byref(u)) == E_ARG
    assert lib.ccm_map_table_correct_frames(None, fake, C.byref(u)) == E_ARG
    assert lib.ccm_map_table_correct_frames(fake, None, C.byref(u)) == E_ARG
    assert lib.ccm_map_table_correct_frames(None, None, None) == E_ARG
    assert (pos == 77).all()


def test_python_mirror_is_exposed():
    from motioncheck_ccm_slam_amd import tracking
    sig = inspect.signature(tracking.MapPointTable.correct)
    assert list(sig.parameters)[1:] == ["kfs", "n_moved", "slot", "owner", "sim3_before", "sim3_after", "Tcw_after", "Ow_after", "in_order",
                                        "lists", "fetch"]
    assert sig.parameters["in_order"].default is False and sig.parameters["fetch"].default is True and sig.parameters["lists"].default is None


# ------------------------------------------------------------------------------------------------------------ known answers
def test_new_pose_equals_pose_to_camera():
    """[R | t * (1.0 / s)] of the corrected Sim3 through ccm_pose_to_camera (the host's definition, csrc/pose_camera.h), byte for byte."""
    Cs = MC.scene(1)
    rng = np.random.default_rng(5)
    cases = list(Cs["sim3_after"]) + [np.concatenate([q / np.linalg.norm(q), t, [s]]) for q, t, s in
                                      zip(rng.normal(size=(40, 4)), rng.normal(0, 3, (40, 3)), np.exp(rng.uniform(-1, 1, 40)))]
    for S in cases:
        T, Ow = MC.new_pose(S)
        Tl, Ol = pose_to_camera(np.concatenate([S[:4], S[4:7] * (1.0 / S[7])]))
        assert T.tobytes() == Tl.tobytes() and Ow.tobytes() == Ol.tobytes()
    T, Ow = MC.new_pose([0, 0, 0, 1, 2, -4, 6, 2])                # identity rotation, scale 2: t / 2, Ow = -t / 2
    assert (T == np.array([[1, 0, 0, 1], [0, 1, 0, -2], [0, 0, 1, 3]], "f4")).all() and (Ow == np.array([-1, 2, -3], "f4")).all()


def test_one_owner_poses_first_equals_the_array_route_narrowed():
    Cs = MC.scene(1)
    S = Cs["S"]; rows = _rows(Cs)
    n = len(S["slot"])
    for k in (0, MC.N_MOVED - 1):
        owner = np.full(n, k, "i4")
        got = MC.correct(Cs, rows, MC.SIM3, MC.POSES_FIRST, lists=False, owner=owner)
        want = correct_map_points_ref(rows["pos"].astype("f8"), owner, Cs["sim3_before"], Cs["sim3_after"]).astype("f4")
        assert got["pos"].tobytes() == want.tobytes() and (got["pos"] != rows["pos"]).any(1).all()
        assert got["normal"].tobytes() == rows["normal"].tobytes()       # without lists the other columns stay
    none = MC.correct(Cs, rows, MC.SIM3, MC.POSES_FIRST, owner=np.full(n, -1, "i4"))
    for k in ("pos", "normal", "min_dist", "max_dist"):
        assert none[k].tobytes() == rows[k].tobytes(), k


def test_rigid_known_answers():
    """A keyframe at Ow = (1, 2, 3) with identity rotation moves to Ow' = (0, 0, 1) with a quarter turn about z: the point keeps its
    camera coordinates."""
    Tb = np.array([[1, 0, 0, -1], [0, 1, 0, -2], [0, 0, 1, -3]], "f4")
    Ta = np.array([[0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 1, -1]], "f4")          # Rcw = Rz(-90 deg), tcw = -Rcw Ow'
    Oa = np.array([0, 0, 1], "f4")
    P = np.array([[2, 2, 7], [5, 5, 5]], "f4")
    out = MC.rigid_positions(P, np.array([0, -1]), [Tb], [Ta.reshape(12)], [Oa])
    Xc = np.array([1, 0, 4], "f4")                                # P - Ow
    assert (out[0] == Ta[:, :3].T @ Xc + Oa).all() and (out[0] == np.array([0, 1, 5], "f4")).all() and (out[1] == P[1]).all()


# ------------------------------------------------------------------------------------------------------------ scene
def test_scene_conditions():
    Cs = MC.scene(1)
    S = Cs["S"]; rows = _rows(Cs)
    owner, c = Cs["owner"], S["counts"]
    assert Cs["n_moved"] == 5 and len(S["kfs"]) == 8 and len(owner) == 400
    assert 0.1 < (owner < 0).mean() < 0.3 and set(owner[owner >= 0]) == set(range(5))
    for want in (0, 1, 63, 64, 65, 130, 300):
        assert (c == want).any(), want
    for want in MC.EDGE_COUNTS:
        assert (owner[c == want] >= 0).all(), want
    assert (c[owner >= 0] == 0).sum() >= 5                        # points that move and keep their normal
    assert (np.isin(S["obs_kf"], (5, 6, 7))).mean() > 0.2         # keyframes that are observed and never moved
    new_Ow = np.stack([MC.new_pose(s)[1] for s in Cs["sim3_after"]])
    old_Ow = np.stack([k["Ow"] for k in S["kfs"][:5]])
    assert (np.abs(new_Ow - old_Ow).max(1) > 0.05).all()
    a = MC.correct(Cs, rows, MC.SIM3, MC.IN_ORDER)
    b = MC.correct(Cs, rows, MC.SIM3, MC.POSES_FIRST)
    assert a["pos"].tobytes() == b["pos"].tobytes() and a["Tcw"].tobytes() == b["Tcw"].tobytes()
    many = (owner >= 0) & (c >= 2)
    differ = (a["normal"].view("u4") != b["normal"].view("u4")).any(1)
    print("order rule: normals differ on %d of %d owned points with >= 2 observations" % (differ[many].sum(), many.sum()))
    assert differ[many].sum() > 0.5 * many.sum()
    assert not differ[(owner < 0) | (c == 0)].any()
    moved = owner >= 0
    assert (a["pos"][moved] != rows["pos"][moved]).any(1).all() and a["pos"][~moved].tobytes() == rows["pos"][~moved].tobytes()
    for k in ("normal", "min_dist", "max_dist"):                  # rows that keep their normal and depth
        keep = ~moved | (c == 0)
        assert a[k][keep].tobytes() == rows[k][keep].tobytes(), k
    r = MC.correct(Cs, rows, MC.RIGID, MC.POSES_FIRST, lists=False)
    assert (r["pos"][moved] != rows["pos"][moved]).any(1).all() and r["normal"].tobytes() == rows["normal"].tobytes()
    assert r["Tcw"].tobytes() == a["Tcw"].tobytes()
