"""The kernels and host loops that walk the vocabulary tree or a FeatureVector (k_voc_transform and the tree layout of ccm_voc_create,
ccm_bow_vector, ccm_bow_score_l1, k_distinctive, k_bow_directory, k_bow_greedy / k_bow_filter / k_bow_groups / k_bow_invert and their
batched forms, ccm_search_for_triangulation over k_hamming_ranges, k_cnmp_match, k_cnmp_match_frames) against tests/bow_ref.py, the
definition restated from the reference's text, on the hand-built cases of tests/bow_cases.py: ties between children, between rows
and between candidates, distances at the thresholds, the ratio test at equality, taken and invalid candidates, node ranges around the
64-lane stride, histogram bins on x.5.  Every comparison is exact: integers, and float64 values for the BowVector and the score.

Every case goes through each entry point that realises it: ORBVocabulary.transform_features and transform_features_dev,
ccm_bow_vector, score, distinctive_descriptors, DeviceFrame.compute_bow with bow() against set_bow (every descent case at every
levelsup, so that the vocabulary's own `weight > 0` meets 0.0, -0.0, a negative weight and 5e-324, below and above the 4096 features
at which the directory moves from the device to the host; and the grid vocabulary's cases), ORBmatcher.SearchByBoW,
SearchByBoWHandle and SearchByBoWFrames, SearchForTriangulation, and tap.match of LocalMapping.CreateNewMapPoints in the array form
and in the frame-handle form (which exposes the same tap).  A frame handle refuses node ids of 2^24 and above: for those directory
patterns only the refusal is checked here, the pattern itself is held to the definition on the CPU.  One context serves everything;
the small cases run again after a large call of each kind, so that a reused staging buffer cannot hide a stale value."""
import numpy as np
import pytest

import bow_cases as C
import bow_ref as R
import frame_bow_ref as fb
from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.frame import DeviceFrame
from motioncheck_ccm_slam_amd.mapping import LocalMapping, MapKeyFrame
from motioncheck_ccm_slam_amd.matcher import FrameGridView, ORBmatcher
from motioncheck_ccm_slam_amd.vocabulary import ORBVocabulary, synthetic_tree

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in C.all_cases()}
K_CAM = np.array([458.0, 458.0, 376.0, 240.0], "f4")


def norm(o):
    if isinstance(o, (list, tuple)):
        return [norm(x) for x in o]
    if isinstance(o, np.ndarray):
        return o.tolist()
    return o.item() if isinstance(o, np.generic) else o


@pytest.fixture(scope="module")
def want():
    """The definition's answer per case, computed once."""
    cache = {}

    def get(case):
        if case["name"] not in cache:
            cache[case["name"]] = norm(C.run_ref(case))
        return cache[case["name"]]
    return get


def _bow_vector(wid, w, nid, weighting=R.TF_IDF, scoring=R.L1_NORM):
    lib = _lib.load()
    n = len(wid)
    wid = np.ascontiguousarray(wid, "i4"); w = np.ascontiguousarray(w, "f8"); nid = np.ascontiguousarray(nid, "i4")
    oid = np.zeros(max(n, 1), "i4"); oval = np.zeros(max(n, 1), "f8"); fv = np.full(max(n, 1), -1, "i4")
    m = lib.ccm_bow_vector(n, _lib.ptr(wid), _lib.ptr(w), _lib.ptr(nid), int(weighting), int(scoring), _lib.ptr(oid), _lib.ptr(oval), _lib.ptr(fv))
    assert m >= 0
    return oid[:m].copy(), oval[:m].copy(), fv[:n].copy()


def _transform_both(voc, feats, levelsup):
    """transform_features from host rows and transform_features_dev from device rows: one answer."""
    import torch
    got = norm(voc.transform_features(feats, levelsup))
    if len(feats):
        dev = torch.from_numpy(np.ascontiguousarray(feats)).cuda()
        torch.cuda.synchronize()
        assert norm(voc.transform_features_dev(dev.data_ptr(), len(feats), levelsup)) == got
    return got


def _plain_frame(ctx, desc, angle=None):
    """A handle over descriptors alone: the keypoints play no part in anything tested here."""
    n = len(desc)
    i = np.arange(n)
    return DeviceFrame(FrameGridView((i % 700 + 10).astype("f4"), (i % 400 + 10).astype("f4"), np.zeros(n, "i4"), desc),
                       None if angle is None else np.ascontiguousarray(angle, "f4"), ctx=ctx)


def _same_dir(got, want):
    assert norm(got) == norm(want)
    for g in got:
        assert g.dtype == np.int32


def _run_bow(ctx, case):
    a = case["args"]
    kfkf = a["kfkf"]
    m = ORBmatcher(a["nnratio"], a["check_ori"], ctx=ctx)
    n1, n2 = len(a["desc1"]), len(a["desc2"])
    out = None
    if n2:
        n, m12 = m.SearchByBoW(a["desc1"], a["node1"], a["valid1"], a["angle1"], a["desc2"], a["node2"], a["angle2"], valid2=a["valid2"])
        out = [n, m12] if kfkf else [n, m12, fb.invert(m12, n2)]
    with _plain_frame(ctx, a["desc1"], a["angle1"]) as h1, _plain_frame(ctx, a["desc2"], a["angle2"]) as h2:
        h1.set_bow(a["node1"]); h2.set_bow(a["node2"])
        if kfkf:
            nm, b12 = m.SearchByBoWFrames(h1, [h2], a["valid1"], [a["valid2"]])
            got = [int(nm[0]), b12[0]]
        else:
            mark = (np.arange(n2) + 5).astype("i4")
            h2.map_points = mark
            n, match = m.SearchByBoWHandle(h1, h2, a["valid1"], min_matches=n1 + n2 + 1)
            assert (h2.map_points == mark).all()
            got = [n, fb.invert(match, n1), match]                    # match12 back from the per-frame-feature form
    assert out is None or norm(out) == norm(got)
    return got


def _kf(a, side):
    if side == 1:
        n = len(a["desc1"])
        return dict(kp_x=a["x1"], kp_y=a["y1"], kp_octave=np.zeros(n, "i4"), desc=a["desc1"], node=a["node1"], has_mp=a["has_mp1"], K=K_CAM,
                    Tcw=np.eye(4, dtype="f4")[:3], Ow=np.zeros(3, "f4"), scale_factors=C.SF2, level_sigma2=C.SIG2)
    T = np.eye(4, dtype="f4")[:3].copy(); T[0, 3] = -1.0
    return dict(kp_x=a["x2"], kp_y=a["y2"], kp_octave=a["octave2"], desc=a["desc2"], node=a["node2"], has_mp=a["has_mp2"], K=K_CAM, Tcw=T,
                Ow=np.array([1.0, 0.0, 0.0], "f4"), scale_factors=C.SF2, level_sigma2=C.SIG2)


def _handle(ctx, d):
    f = DeviceFrame(FrameGridView(d["kp_x"], d["kp_y"], d["kp_octave"], d["desc"]), ctx=ctx)
    f.map_points = np.where(np.asarray(d["has_mp"]) != 0, np.arange(len(d["has_mp"])), -1).astype("i4")
    f.set_camera(d["K"], d["scale_factors"], d["level_sigma2"])
    f.set_bow(d["node"])
    f.set_pose(d["Tcw"], d["Ow"])
    return f


def _run_tri(ctx, case):
    a = case["args"]
    m = ORBmatcher(0.6, a["check_ori"], ctx=ctx)
    n, m12 = m.SearchForTriangulation(*[a[k] for k in ("desc1", "node1", "has_mp1", "x1", "y1", "angle1", "desc2", "node2", "has_mp2", "x2", "y2", "angle2",
                                                         "octave2", "F12", "ex", "ey", "scale_factors2", "level_sigma2_2")])
    if not a["check_ori"]:                                          # CreateNewMapPoints matches without the orientation filter (Mapping.cpp:312)
        cur, nb = _kf(a, 1), _kf(a, 2)                              # baseline 1 m over a median depth of 1 m: the neighbour is not skipped
        mk = lambda d: MapKeyFrame(d["kp_x"], d["kp_y"], d["kp_octave"], d["desc"], d["node"], d["has_mp"], d["K"], d["Tcw"], d["Ow"], d["scale_factors"],
                                   d["level_sigma2"])
        lm = LocalMapping(ctx=ctx)
        F12 = a["F12"].reshape(1, 3, 3); epi = np.array([[a["ex"], a["ey"]]], "f4")
        lm.CreateNewMapPoints(mk(cur), [mk(nb)], [1.0], F12=F12, epipole=epi)
        assert (lm.tap()["match"][0] == m12).all()
        h1, h2 = _handle(ctx, cur), _handle(ctx, nb)
        try:
            lm.CreateNewMapPointsFrames(h1, [h2], [1.0], F12, epi)
            assert (lm.tap()["match"][0] == m12).all()
        finally:
            h1.close(); h2.close()
    return [n, m12]


def _compute_bow(ctx, voc, feats, levelsup, wid, w, fv):
    """DeviceFrame.compute_bow on a handle of these descriptors: its outputs against (wid, w, fv) of the array calls, the directory it
    builds against set_bow(fv) on a second handle and against the form that reads nothing back on a third.  -> the directory."""
    with _plain_frame(ctx, feats) as f, _plain_frame(ctx, feats) as g, _plain_frame(ctx, feats) as q:
        assert norm(f.compute_bow(voc, levelsup)) == norm([wid, w, fv])
        d = f.bow()
        g.set_bow(fv)
        _same_dir(g.bow(), d)
        assert q.compute_bow(voc, levelsup, outputs=False) is None
        _same_dir(q.bow(), d)
    return d


def run_gpu(ctx, case):
    """A case through every entry point of its kind; the entry points must agree with one another, the answer goes to the caller."""
    k, a = case["kind"], case.get("args")
    if k == "descent":
        voc = ORBVocabulary(a["k"], a["L"], a["parent"], a["desc"], a["weight"], ctx=ctx)
        assert voc.size() == int((np.bincount(a["parent"][1:], minlength=len(a["parent"])) == 0)[1:].sum())
        out = []
        for lu in a["levelsups"]:
            wid, w, nid = _transform_both(voc, a["feats"], lu)
            fv = _bow_vector(wid, w, nid)[2]
            out.append([wid, w, nid, fv] + list(_compute_bow(ctx, voc, a["feats"], lu, wid, w, fv)))
        return out
    if k == "grid":
        v = a["voc"]
        voc = ORBVocabulary(v["k"], v["L"], v["parent"], v["desc"], v["weight"], ctx=ctx)
        wid, w, nid = voc.transform_features(a["feats"], a["levelsup"])
        fv = _bow_vector(wid, w, nid)[2]
        return [wid, w, fv] + list(_compute_bow(ctx, voc, a["feats"], a["levelsup"], wid, w, fv))
    if k == "bowvec":
        return [_bow_vector(a["word_id"], a["weight"], a["node_id"], wt, sc) for wt, sc in C.COMBOS]
    if k == "score":
        voc = ORBVocabulary(2, 1, [0, 0], np.zeros((2, 32), np.uint8), [0.0, 1.0], ctx=ctx)
        return [voc.score(x, y) for x, y in a["pairs"]]
    if k == "distinctive":
        voc = ORBVocabulary(2, 1, [0, 0], np.zeros((2, 32), np.uint8), [0.0, 1.0], ctx=ctx)
        desc, first, count = C.pool(a["groups"])
        assert len(first) < 2 or (np.diff(first) <= 0).all()        # `first` descends
        return voc.distinctive_descriptors(desc, first, count)
    if k == "directory":
        out = []
        for node in a["patterns"].values():
            with _plain_frame(ctx, np.zeros((len(node), 32), np.uint8)) as f:
                if len(node) and node.max() > C.HANDLE_BIG:            # a handle takes node ids below 2^24 and says so; its bow stays
                    f.set_bow(np.zeros(len(node), "i4"))
                    with pytest.raises(_lib.CcmError, match="not below 16777216"):
                        f.set_bow(node)
                    assert norm(f.bow()) == norm(R.feature_vector(np.zeros(len(node), "i4")))
                    out.append(None)                                   # nothing to compare: the caller leaves this pattern out
                    continue
                f.set_bow(node)
                d = f.bow()
                assert all(x.dtype == np.int32 for x in d)
                out.append(d)
        return out
    if k == "bow":
        return _run_bow(ctx, case)
    if k == "bow_batch":
        subs = case["subs"]
        a0 = subs[0]["args"]
        m = ORBmatcher(a0["nnratio"], a0["check_ori"], ctx=ctx)
        hs = [_plain_frame(ctx, s["args"]["desc2"], s["args"]["angle2"]) for s in subs]
        try:
            with _plain_frame(ctx, a0["desc1"], a0["angle1"]) as h1:
                h1.set_bow(a0["node1"])
                for h, s in zip(hs, subs):
                    h.set_bow(s["args"]["node2"])
                nm, m12 = m.SearchByBoWFrames(h1, hs, a0["valid1"], [s["args"]["valid2"] for s in subs])
        finally:
            for h in hs:
                h.close()
        for k2, s in enumerate(subs):                               # and the single calls
            if len(s["args"]["desc2"]):
                assert norm(_run_bow(ctx, s)) == norm([int(nm[k2]), m12[k2]])
        return [[int(nm[k2]), m12[k2]] for k2 in range(len(subs))]
    assert k == "tri"
    return _run_tri(ctx, case)


def _check(ctx, want, case):
    got, ref = norm(run_gpu(ctx, case)), want(case)
    if case["kind"] == "directory":                                 # the patterns a handle refuses (ids of 2^24 and above) gave nothing
        assert len(got) == len(ref)
        ref = [r for g, r in zip(got, ref) if g is not None]
        got = [g for g in got if g is not None]
        assert got
    assert got == ref, case["name"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_equals_the_definition(ctx, want, name):
    _check(ctx, want, CASES[name])


@pytest.fixture(scope="module")
def large():
    """One large input of each kind with the definition's answer, made once on the CPU: 5000 features down the ragged 10-way tree, and
    400 x 600 descriptors in ONE node (a group of 600) for both SearchByBoW forms and for SearchForTriangulation."""
    tr = synthetic_tree(10, 4, seed=5, ragged=True)
    feats = fb.features(tr, np.random.default_rng(0), 5000)
    rng = np.random.default_rng(7)
    d1, d2 = synth.descriptor_pair(5)
    d1, d2 = d1[:400], d2[:600]
    v1 = rng.random(400) < 0.8; v2 = rng.random(600) < 0.9
    a1 = rng.uniform(0, 360, 400).astype("f4"); a2 = rng.uniform(0, 360, 600).astype("f4")
    z1 = np.zeros(400, "i4"); z2 = np.zeros(600, "i4")
    bow = [((d1, z1, v1, a1, d2, z2, a2, v2 if kfkf else None), R.search_by_bow(d1, z1, v1, a1, d2, z2, a2, v2 if kfkf else None, 0.7, True, kfkf))
           for kfkf in (False, True)]
    x = rng.uniform(0, 752, 600).astype("f4"); y = rng.uniform(0, 480, 600).astype("f4")
    has1 = rng.random(400) < 0.4; has2 = rng.random(600) < 0.3
    F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], "f4")
    tri = (d1, z1, has1, x[:400], y[:400], a1, d2, z2, has2, x, y + 0.5, a2, rng.integers(0, 2, 600), F12, 300.0, 240.0, C.SF2, np.array([1.0, 1.44], "f4"))
    return dict(tree=tr, feats=feats, transform=norm(R.Vocabulary(10, 4, *tr).transform_features(feats, 2)), bow=bow, tri=tri,
                tri_ref=R.search_for_triangulation(*tri, True))


def test_large_calls_equal_the_definition(ctx, large):
    """The calls that grow the staging buffers, each held to the definition; the small cases follow in the next test."""
    voc = ORBVocabulary(10, 4, *large["tree"], ctx=ctx)
    assert _transform_both(voc, large["feats"], 2) == large["transform"]
    for args, ref in large["bow"]:
        n, m12 = ORBmatcher(0.7, True, ctx=ctx).SearchByBoW(*args[:7], valid2=args[7])
        assert n == ref[0] and (m12 == ref[1]).all() and n > 20
    n, m12 = ORBmatcher(0.6, True, ctx=ctx).SearchForTriangulation(*large["tri"])
    assert n == large["tri_ref"][0] and (m12 == large["tri_ref"][1]).all()
    big = np.tile(np.arange(40, dtype=np.uint8)[:, None], (1, 32))
    voc.distinctive_descriptors(np.tile(big, (50, 1)), np.arange(50) * 40, np.full(50, 40))


@pytest.mark.parametrize("kind", ["descent", "bowvec", "score", "distinctive", "directory", "bow", "bow_batch", "tri"])
def test_small_cases_again_after_large_calls(ctx, want, kind):
    """Every small case of a kind once more on the same context, behind the large calls of the test above: what those left in the
    staging buffers must not show."""
    for name in sorted(CASES):
        if CASES[name]["kind"] == kind:
            _check(ctx, want, CASES[name])
