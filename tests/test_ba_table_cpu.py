"""Local BA on the table (include/ccm_hot.h), what can be held without a GPU: the three symbols and their mirror, the NULL-argument
answers, ccm_pose_to_camera against the rule Tracking.camera states, and the test helper's own bookkeeping (tests/ba_table_case.py):
the five graphs of the GPU tests survive the trip through float32 features and the eight-entry level table exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import ba_table_case as B
from motioncheck_ccm_slam_amd import _lib, optimizer
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.optimizer import Optimizer, pose_to_camera, pose_to_mat4f
from motioncheck_ccm_slam_amd.tracking import Tracking

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ccm_ba_solve_table_frames", "ccm_pose_to_camera", "ccm_frame_get_pose")
E_ARG = -1


def test_symbols_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "ccm_hot.h")).read()
    lib = _lib.load()
    for s in NEW:
        assert s + "(" in header and s in _lib.SYMBOLS and hasattr(lib, s)
    assert "} ccm_ba_table_problem;" in header and "#define CCM_ABI_VERSION 3" in header
    # the struct mirrors the header field for field (names in declaration order)
    body = header.split("} ccm_ba_table_problem;")[0].rsplit("typedef struct {", 1)[1]
    names = [f[0] for f in _lib.BaTableProblem._fields_]
    at = [body.index(" " + n + ";") for n in names]
    assert at == sorted(at) and len(names) == 14
    assert C.sizeof(_lib.BaTableProblem) == 14 * 8
    assert callable(Optimizer.LocalBundleAdjustmentClientTable) and callable(Optimizer.BundleAdjustmentClientTable)
    assert callable(optimizer.pose_to_camera) and callable(DeviceFrame.pose)


def test_null_arguments_need_no_device():
    lib = _lib.load()
    pb = _lib.BaTableProblem(); opt = _lib.BaOptions(); res = _lib.BaResult()
    fake = C.c_void_p(8)                                         # never dereferenced: a NULL neighbour answers first
    assert lib.ccm_ba_solve_table_frames(None, fake, C.byref(pb), C.byref(opt), C.byref(res)) == E_ARG
    assert lib.ccm_ba_solve_table_frames(fake, None, C.byref(pb), C.byref(opt), C.byref(res)) == E_ARG
    assert lib.ccm_ba_solve_table_frames(fake, fake, None, C.byref(opt), C.byref(res)) == E_ARG
    T = np.zeros(12, "f4"); O = np.zeros(3, "f4"); p = np.zeros(7)
    assert lib.ccm_pose_to_camera(None, _lib.ptr(T), _lib.ptr(O)) == E_ARG
    assert lib.ccm_pose_to_camera(_lib.ptr(p), None, _lib.ptr(O)) == E_ARG
    assert lib.ccm_frame_get_pose(None, _lib.ptr(T), _lib.ptr(O)) == E_ARG


def test_pose_to_camera_is_the_rule_tracking_states():
    rng = np.random.default_rng(5)
    q = rng.normal(size=(1000, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 3] < 0] *= -1
    poses = np.concatenate([q, rng.uniform(-5, 5, (1000, 3))], 1)
    poses[0] = [0, 0, 0, 1, 0, 0, 0]                             # the identity
    poses[1] = [0, 1, 0, 0, 0.5, -2.0, 3.0]                      # 180 degrees about y
    poses[2] = [1, 0, 0, 0, -1.0, 0.25, 0.0]                     # 180 degrees about x
    for p in poses:
        T, O = pose_to_camera(p)
        Tr, Or = Tracking.camera(pose_to_mat4f(p))
        assert T.dtype == np.float32 and O.dtype == np.float32
        assert T.tobytes() == Tr.tobytes() and O.tobytes() == Or.tobytes()


@pytest.mark.parametrize("name", list(B.GRAPHS))
def test_helper_arrays_are_the_graph_widened(name):
    g = B.graph(name)
    P, L, E = B.GRAPHS[name][1]
    assert (len(g["poses"]), len(g["points"]), len(g["edge_pose"])) == (P, L, E)
    # the generator's observations are float32-exact and its information values lie in the table
    assert (g["obs"].astype("f4").astype("f8") == g["obs"]).all()
    B.octaves(g["info"])
    Lst = B.lists(g)
    A, o = Lst["arrays"], Lst["order"]
    assert (A["obs"] == g["obs"][o]).all() and (A["info"] == g["info"][o]).all()
    assert (A["edge_pose"] == g["edge_pose"][o]).all() and (A["edge_point"] == g["edge_point"][o]).all()
    assert (A["points"] == g["points"].astype("f4").astype("f8")).all()
    # the layout is what it claims: a feature index is not the edge index, the slots are no identity, the lists are not sorted
    assert (Lst["obs_feat"] != np.arange(E)).any()
    assert len(np.unique(Lst["slot"])) == L and Lst["capacity"] >= 2 * L
    d = np.diff(A["edge_pose"].astype("i8")); same = np.diff(A["edge_point"]) == 0
    assert (np.diff(A["edge_point"]) >= 0).all() and (d[same] < 0).any()
    assert (np.diff(Lst["obs_first"]) == np.bincount(g["edge_point"], minlength=L)).all()
    for k, f in enumerate(Lst["feats"]):
        assert len(f["kx"]) == (g["edge_pose"] == k).sum() + B.PAD
