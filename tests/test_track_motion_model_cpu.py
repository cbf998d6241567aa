"""ccm_frame_track_motion_model (include/ccm_hot.h "map-point table") without a GPU: the numpy restatement against a plain float64
projection and against a hand-made case with a known answer, the ctypes mirrors of its two structs against the header as the C
compiler lays it out, and the export."""
import ctypes as C
import os
import subprocess

import numpy as np

import search_local_points_ref as R
import track_motion_model_ref as M
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.matcher import FrameGridView

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_ref_projection_agrees_with_a_float64_pinhole():
    rows = R.random_points(5000, 11)
    Tcw, _ = R.camera()
    reason, u, v, Pc = M.project(rows["pos"], Tcw)
    T = Tcw.astype("f8"); P = rows["pos"].astype("f8")
    Pd = P @ T[:, :3].T + T[:, 3]
    fx, fy, cx, cy = R.INTR
    ud = fx * Pd[:, 0] / Pd[:, 2] + cx; vd = fy * Pd[:, 1] / Pd[:, 2] + cy
    ok = reason == M.QUERY
    assert ok.sum() > 500 and (Pc[:, 2] != 0).all()
    # float32 keeps 24 bits: a coordinate below 1024 px is good to 1024 * 2^-24 per rounding, and fewer than ten roundings separate
    # the two forms
    assert np.abs(u[ok] - ud[ok]).max() <= 1e-3 and np.abs(v[ok] - vd[ok]).max() <= 1e-3
    inside = (Pd[:, 2] > 0) & (ud >= 0) & (ud <= 752) & (vd >= 0) & (vd <= 480)
    near = (np.abs(ud) < 1e-2) | (np.abs(ud - 752) < 1e-2) | (np.abs(vd) < 1e-2) | (np.abs(vd - 480) < 1e-2) | (np.abs(Pd[:, 2]) < 1e-4)
    assert (ok == inside)[~near].all()
    assert (u[~ok] == 0).all() and (v[~ok] == 0).all()
    assert {M.BEHIND, M.U_OUT, M.V_OUT} <= set(reason.tolist())


def _hand_made():
    """Identity camera.  Last-frame feature 0 holds a point behind the camera, 1 a point that projects exactly onto u == max_x, 2 a
    point in front of the principal point; the current frame has a feature with that point's descriptor there, and an unrelated one."""
    edge = R.edge_points()
    rng = np.random.default_rng(3)
    desc = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    rows = dict(pos=np.array([[0.1, 0.1, -1.0], edge["pos"][1], [0.0, 0.0, 2.0]], "f4"), desc=desc,
                flags=np.array([R.LIVE | R.HAS_OBS, R.LIVE | R.HAS_OBS, R.LIVE | R.HAS_OBS], np.uint8))
    cur = FrameGridView([R.INTR[2], 100.0], [R.INTR[3], 100.0], [0, 0], np.stack([desc[2], ~desc[2]]))
    return rows, cur


def test_replay_on_a_hand_made_case(oracle):
    rows, cur = _hand_made()
    Tcw = R.IDENTITY[0]
    last_ids = np.array([0, 1, 2], "i4")
    q = M.queries(last_ids, rows, Tcw)
    assert q["reason"].tolist() == [M.BEHIND, M.QUERY, M.QUERY]
    assert q["u"][1] == F(R.BOUNDS[1]) and q["v"][1] == F(R.INTR[3])          # on the bound: inside
    assert q["u"][2] == F(R.INTR[2]) and q["v"][2] == F(R.INTR[3]) and q["u"][0] == 0
    ang = np.zeros(2, "f4"); lang = np.zeros(3, "f4"); loct = np.zeros(3, "i4")
    args = (oracle, cur, ang, loct, lang, last_ids, rows, Tcw, R.SCALE)
    r = M.replay(*args)                                                        # one match: retried, then below the threshold
    assert (r["n_matches"], r["passes"], r["pass_matches"], r["posed"]) == (1, 2, [1, 1], False)
    assert r["match"].tolist() == [2, -1] and r["mp_id"].tolist() == [2, -1] and r["n_matches_map"] == 1
    pose = lambda ids: (np.arange(7.0), np.array([0, 0], np.uint8), 1)         # noqa: E731
    r = M.replay(*args, pose=pose, retry_below=0, min_matches=1)               # posed, nothing discarded
    assert (r["passes"], r["posed"], r["n_inliers"], r["n_matches_map"]) == (1, True, 1, 1) and r["mp_id"].tolist() == [2, -1]
    drop = lambda ids: (np.arange(7.0), np.array([1, 1], np.uint8), 0)         # noqa: E731
    r = M.replay(*args, pose=drop, retry_below=0, min_matches=1)               # the match is an outlier: discarded
    assert r["posed"] and r["mp_id"].tolist() == [-1, -1] and r["n_matches_map"] == 0 and r["outlier"].tolist() == [1, 1]
    r = M.replay(*args, last_outlier=[0, 0, 1])                                # LastFrame.mvbOutlier: no query
    assert r["reason"].tolist() == [M.BEHIND, M.QUERY, M.LAST_OUTLIER] and r["n_matches"] == 0 and r["mp_id"].tolist() == [-1, -1]
    rows["flags"][2] = R.LIVE                                                  # a point without observations is matched, not counted
    r = M.replay(*args)
    assert r["mp_id"].tolist() == [2, -1] and r["n_matches_map"] == 0
    r = M.replay(oracle, cur, ang, loct[:0], lang[:0], last_ids[:0], rows, Tcw, R.SCALE)
    assert r["passes"] == 0 and r["n_matches"] == 0 and r["mp_id"].tolist() == [-1, -1]


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ccm_hot.h"
#define P(T, f) printf(#T "." #f " %d\n", (int)offsetof(T, f))
int main(void)
{
    printf("ccm_tmm_params %d\nccm_tmm_result %d\n", (int)sizeof(ccm_tmm_params), (int)sizeof(ccm_tmm_result));
    P(ccm_tmm_params, Tcw); P(ccm_tmm_params, fx); P(ccm_tmm_params, fy); P(ccm_tmm_params, cx); P(ccm_tmm_params, cy);
    P(ccm_tmm_params, min_x); P(ccm_tmm_params, max_x); P(ccm_tmm_params, min_y); P(ccm_tmm_params, max_y); P(ccm_tmm_params, n_levels);
    P(ccm_tmm_params, scale_factors); P(ccm_tmm_params, th); P(ccm_tmm_params, retry_below); P(ccm_tmm_params, min_matches);
    P(ccm_tmm_params, check_ori); P(ccm_tmm_params, orb_dist); P(ccm_tmm_params, last_outlier); P(ccm_tmm_params, inv_level_sigma2);
    P(ccm_tmm_params, intr);
    P(ccm_tmm_result, n_matches); P(ccm_tmm_result, passes); P(ccm_tmm_result, posed); P(ccm_tmm_result, n_inliers);
    P(ccm_tmm_result, n_matches_map); P(ccm_tmm_result, pose7); P(ccm_tmm_result, match); P(ccm_tmm_result, mp_id);
    P(ccm_tmm_result, outlier); P(ccm_tmm_result, u); P(ccm_tmm_result, v); P(ccm_tmm_result, valid);
    return 0;
}
"""


def test_struct_mirrors_equal_the_compiled_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    want = dict((k, int(v)) for k, v in (line.split() for line in out.stdout.splitlines()))
    got = {}
    for name, T in (("ccm_tmm_params", _lib.TmmParams), ("ccm_tmm_result", _lib.TmmResult)):
        got[name] = C.sizeof(T)
        for f, _ in T._fields_:
            got["%s.%s" % (name, f)] = getattr(T, f).offset
    assert got == want and len(want) == 2 + 19 + 12


def test_entry_point_is_declared_exported_and_refuses_null():
    lib = _lib.load()
    assert "ccm_frame_track_motion_model" in _lib.SYMBOLS and hasattr(lib, "ccm_frame_track_motion_model")
    assert len(lib.ccm_frame_track_motion_model.argtypes) == 6
    assert lib.ccm_abi_version() == 3 == _lib.ABI_VERSION         # an export was added, nothing changed
    p, r = _lib.TmmParams(), _lib.TmmResult()
    assert lib.ccm_frame_track_motion_model(None, None, None, None, C.byref(p), C.byref(r)) == -1
    from motioncheck_ccm_slam_amd.tracking import MotionModelResult, Tracking
    assert callable(Tracking.TrackWithMotionModel) and MotionModelResult(posed=1, n_matches_map=10).ok
