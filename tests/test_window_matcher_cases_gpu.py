"""The windowed-matcher kernels (k_window_candidates, k_window_select, k_window_greedy<0|1|2>) and the host loops beside them against
tests/window_matcher_ref.py, the definition restated from the reference's text, on the hand-built frames of
tests/window_matcher_cases.py: ties decided by visiting order, distances at the thresholds, the ratio test at equality, windows
whose edge falls on a feature, stale histogram entries, and every size boundary of the kernels (64 lanes, 16 candidates in
registers, 1024 points per batch, the first list capacity of 64).  Everything is an integer decision: exact equality, no case set
aside."""
import os
import subprocess
import sys

import numpy as np
import pytest

import window_matcher_cases as C
import window_matcher_ref as R
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in C.all_cases()}
HANDLE_KINDS = ("projection", "frame")


def norm(o):
    if isinstance(o, (list, tuple)):
        return [norm(x) for x in o]
    if isinstance(o, np.ndarray):
        return o.tolist()
    return o.item() if isinstance(o, np.generic) else o


def view(g):
    bounds = {k: g[k] for k in ("min_x", "max_x", "min_y", "max_y") if k in g}
    return FrameGridView(g["kx"], g["ky"], g["octave"], g["desc"], **bounds)


@pytest.fixture(scope="module")
def want():
    """The definition's answer per case, computed once for the array forms, the handle forms and the batches."""
    cache = {}

    def get(case):
        if case["name"] not in cache:
            cache[case["name"]] = norm(C.run_ref(case))
        return cache[case["name"]]
    return get


def run_gpu(ctx, case, handle=False):
    """A case through the library's entry point of its kind (handle: the frame side as a DeviceFrame, its grid built on the device)."""
    k, a = case["kind"], case["args"]
    if k == "by_sim3":
        return ORBmatcher(ctx=ctx).SearchBySim3(view(case["grid1"]), a["sf1"], view(case["grid2"]), a["sf2"], a["valid1"], a["u1"], a["v1"], a["level1"],
                                                a["mp_desc1"], a["valid2"], a["u2"], a["v2"], a["level2"], a["mp_desc2"], a["th"])
    g = case["grid"]
    fr = view(g)
    if k == "area":
        q = np.array(a["queries"], np.float64)
        nq = len(q)
        ci, cd, cn = ORBmatcher(ctx=ctx).FeaturesInArea(fr, q[:, 0], q[:, 1], q[:, 2], q[:, 3], q[:, 4], np.tile(C.BASE, (nq, 1)), cap=256)
        for i in range(nq):                                          # the distances that ride along: BASE against the listed features
            assert cd[i, :cn[i]].tolist() == [R.hamming(C.BASE, g["desc"][j]) for j in ci[i, :cn[i]]]
        return [ci[i, :cn[i]].tolist() for i in range(nq)]
    if k == "init":
        return ORBmatcher(a["nnratio"], a["check_ori"], ctx=ctx).SearchForInitialization(a["oct1"], a["desc1"], a["angle1"], fr, g["angle"], a["prev_matched"],
                                                                                         a["window"])
    if k == "projection":
        m = ORBmatcher(a["nnratio"], ctx=ctx)
        rest = (a["scale_factors"], a["in_view"], a["level"], a["view_cos"], a["proj_x"], a["proj_y"], a["mp_desc"], a["has_obs"], a["occupied"], a["th"])
        if handle:
            with DeviceFrame(fr, g["angle"], ctx=ctx) as h:
                return m.SearchByProjectionHandle(h, *rest)
        return m.SearchByProjection(fr, *rest)
    if k == "frame":
        m = ORBmatcher(0.9, a["check_ori"], ctx=ctx)
        if handle:
            with DeviceFrame(fr, g["angle"], ctx=ctx) as h:
                return m.SearchByProjectionFrameHandle(h, None, a["scale_factors"], a["valid"], a["u"], a["v"], a["mp_desc"], a["has_obs"], a["occupied"],
                                                       a["th"], last_octave=a["last_octave"], last_angle=a["last_angle"], orb_dist=a["orb_dist"])
        return m.SearchByProjectionFrame(fr, g["angle"], a["scale_factors"], a["valid"], a["u"], a["v"], a["last_octave"], a["last_angle"], a["mp_desc"],
                                         a["has_obs"], a["occupied"], a["th"], orb_dist=a["orb_dist"])
    if k == "sim3":
        return ORBmatcher(ctx=ctx).SearchByProjectionSim3(fr, a["scale_factors"], a["valid"], a["u"], a["v"], a["level"], a["mp_desc"], a["observed"],
                                                          a["matched"], a["th"])
    return ORBmatcher(ctx=ctx).FuseSelect(fr, a["scale_factors"], a["inv_level_sigma2"], a["valid"], a["u"], a["v"], a["level"], a["mp_desc"], a["th"],
                                          a["chi2_check"], a["accept_th"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_array_form_equals_the_definition(ctx, want, name):
    case = CASES[name]
    assert norm(run_gpu(ctx, case)) == want(case)


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["kind"] in HANDLE_KINDS))
def test_handle_form_equals_the_definition(ctx, want, name):
    """ccm_frame_search_by_projection / ccm_frame_search_by_projection_frame: the grid is built by the device, not by the host."""
    case = CASES[name]
    assert norm(run_gpu(ctx, case, handle=True)) == want(case)


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["kind"] in ("projection", "frame", "sim3", "fuse") and not n.startswith("size_")))
def test_candidate_lists_equal_the_definition(ctx, name):
    """ccm_window_candidates on the windows the matcher of the case searches: indices in visiting order, and the distances."""
    case = CASES[name]
    trace = {"windows": []}
    C.run_ref(case, trace=trace)
    w = trace["windows"]
    g = case["grid"]
    a = case["args"]
    qdesc = a["mp_desc"]
    pos = "proj_x" if case["kind"] == "projection" else "u"
    active = a["in_view" if case["kind"] == "projection" else "valid"]
    rows = [i for i in range(len(active)) if active[i]]
    assert len(w) == len(rows)                                      # every active point of these cases searches inside the grid
    assert [float(x[0]) for x in w] == [float(a[pos][i]) for i in rows]
    ci, cd, cn = ORBmatcher(ctx=ctx).FeaturesInArea(view(g), [x[0] for x in w], [x[1] for x in w], [x[2] for x in w], [x[3] for x in w], [x[4] for x in w],
                                                    qdesc[rows], cap=256)
    for q, x in enumerate(w):
        assert ci[q, :cn[q]].tolist() == x[5], q
        assert cd[q, :cn[q]].tolist() == [R.hamming(qdesc[rows[q]], g["desc"][j]) for j in x[5]], q


def test_sim3_batch_equals_the_definition_and_the_single_calls(ctx, want):
    """Keyframe 1's list of 65 makes every keyframe repeat after keyframe 0's workgroup has already set flags."""
    case = C.batch("sim3")
    subs = case["subs"]
    m = ORBmatcher(ctx=ctx)
    per_kf = [tuple(s["args"][k] for k in ("valid", "u", "v", "level", "mp_desc", "observed", "matched")) for s in subs]
    got = m.SearchByProjectionSim3Batch([view(s["grid"]) for s in subs], C.SF, per_kf, subs[0]["args"]["th"])
    assert norm(got) == want(case)
    for s, g in zip(subs, got):
        if len(s["grid"]["kx"]) and len(s["args"]["u"]):
            assert norm(run_gpu(ctx, s)) == norm(g)


def test_fuse_batch_equals_the_definition_and_the_single_calls(ctx, want):
    case = C.batch("fuse")
    subs = case["subs"]
    m = ORBmatcher(ctx=ctx)
    a0 = subs[0]["args"]
    per_kf = [tuple(s["args"][k] for k in ("valid", "u", "v", "level", "mp_desc")) for s in subs]
    views = [view(s["grid"]) for s in subs]
    for chi2 in (False, True):                                      # chi2 on: invSigma2 is all ones and every offset a whole pixel, e2 is exact
        ref = [norm(R.fuse_select(R.Grid(**s["grid"]), *list(s["args"].values())[:8], chi2, a0["accept_th"])) for s in subs]
        if not chi2:
            assert ref == want(case)
        got = m.FuseSelectBatch(views, C.SF, a0["inv_level_sigma2"], per_kf, a0["th"], chi2, a0["accept_th"])
        assert norm(got) == ref
        frames = [DeviceFrame(v, ctx=ctx) for v in views]
        try:
            assert norm(m.FuseSelectBatchFrames(frames, C.SF, a0["inv_level_sigma2"], per_kf, a0["th"], chi2, a0["accept_th"])) == ref
        finally:
            for f in frames:
                f.close()
        for s, v, g in zip(subs, views, got):
            if len(s["grid"]["kx"]) and len(s["args"]["u"]):
                assert norm(m.FuseSelect(v, C.SF, a0["inv_level_sigma2"], *[s["args"][k] for k in ("valid", "u", "v", "level", "mp_desc")], a0["th"], chi2,
                                         a0["accept_th"])) == norm(g)


def test_host_acceptance_loops_equal_the_definition():
    """The acceptance loops on the host (CCM_WINDOW_HOST_ACCEPT=1, the path of problems too large for one workgroup's LDS) are held
    to the same definition: a child process reruns the array, handle and batch tests of this file with the switch set."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CCM_WINDOW_HOST_ACCEPT="1", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", "array_form or handle_form or batch"],
                         env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-1000:]
