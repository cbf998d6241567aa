"""What the frame-BoW tests share: the vocabulary, the synthetic frames of the SearchByBoW cases and the oracle's answers.

Test infrastructure: nothing here is imported by the library.  Everything is made on the CPU, so the properties the GPU tests lean
on (stopped words, a node of more than 64 features, matches the rotation filter drops) are asserted from the oracle alone."""
import numpy as np

from motioncheck_ccm_slam_amd.vocabulary import synthetic_tree

K, L = 10, 4
INTR = np.array([458.0, 457.0, 367.0, 248.0])
POSE0 = np.array([0, 0, 0, 1, 0, 0, 0.0])
N_LEVELS = 8
INV_SIGMA2 = (1.0 / (1.2 ** np.arange(N_LEVELS)) ** 2).astype("f4")


def tree():
    return synthetic_tree(K, L, seed=5, ragged=True)


def features(tr, rng, n):
    """Noisy copies of random nodes' descriptors, a tenth of them random (as tests/test_bow_gpu.py)."""
    par, desc, w = tr
    leaves = rng.integers(1, len(par), n)
    flips = np.packbits(rng.random((n, 256)) < 0.1, axis=1, bitorder="little")
    f = desc[leaves] ^ flips
    f[: n // 10] = rng.integers(0, 256, (n // 10, 32), dtype=np.uint8)
    return np.ascontiguousarray(f, np.uint8)


def words(tr):
    """(stopped words, live words) as node ids: the leaves with weight 0 / > 0."""
    par, desc, w = tr
    leaf = np.bincount(par[1:], minlength=len(par)) == 0
    leaf[0] = False
    return np.flatnonzero(leaf & ~(w > 0)), np.flatnonzero(leaf & (w > 0))


def expected_node(ref_voc, feats, levelsup):
    """(word_id, weight, node with -1 for stopped words) from the oracle's transform"""
    wid, w, nid = ref_voc.transform_features(feats, levelsup)
    return wid, w, np.where(w > 0, nid, -1).astype("i4")


def keypoints(rng, n):
    return rng.uniform(0, 752, n).astype("f4"), rng.uniform(0, 480, n).astype("f4"), rng.integers(0, N_LEVELS, n).astype("i4")


def make_kf(tr, seed, n1):
    """A reference keyframe: dict of desc, angle, kx, ky, oct, ids (mp_id, a fifth of them -1) and xyz (the 3-D point by id)."""
    rng = np.random.default_rng(seed)
    d1 = features(tr, rng, n1)
    a1 = rng.uniform(0, 360, n1).astype("f4")
    kx1, ky1, o1 = keypoints(rng, n1)
    z = rng.uniform(2, 10, n1)
    xyz = np.stack([(kx1 - INTR[2]) / INTR[0] * z, (ky1 - INTR[3]) / INTR[1] * z, z], 1).astype("f4").astype("f8")
    ids = np.where(rng.random(n1) < 0.8, np.arange(n1), -1).astype("i4")
    return dict(desc=d1, angle=a1, kx=kx1, ky=ky1, oct=o1, ids=ids, xyz=xyz)


def make_view(tr, kf, seed, n2, share=0.8, bad_angle=0.15):
    """A frame that sees `share` of the keyframe's features again: descriptors with 3% of the bits flipped, in another order, the
    keypoint angles turned by 20 degrees -- but for `bad_angle` of them, which the rotation histogram drops.  Its keypoints are the
    keyframe's 3-D points seen from a camera 5 cm to the side (a tenth of them moved away: the pose outliers).  -> dict of desc,
    angle, kx, ky, oct, src (feature of kf, or -1) and ids (a mp_id of its own, for the KeyFrame-KeyFrame form)."""
    rng = np.random.default_rng(seed)
    d1, a1, o1, xyz = kf["desc"], kf["angle"], kf["oct"], kf["xyz"]
    n1 = len(d1)
    n_shared = min(int(share * n1), n2)
    src = np.full(n2, -1, "i8")
    src[:n_shared] = rng.permutation(n1)[:n_shared]
    src = src[rng.permutation(n2)]
    has = src >= 0
    d2 = features(tr, rng, n2)
    flips = np.packbits(rng.random((n2, 256)) < 0.03, axis=1, bitorder="little")
    d2[has] = d1[src[has]] ^ flips[has]
    a2 = rng.uniform(0, 360, n2).astype("f4")
    good = has & (rng.random(n2) >= bad_angle)
    a2[good] = np.mod(a1[src[good]] - np.float32(20.0) + rng.normal(0, 2, int(good.sum())).astype("f4"), np.float32(360.0)).astype("f4")
    kx2, ky2, o2 = keypoints(rng, n2)
    P = xyz[src[has]] + np.array([0.05, 0.02, 0.0])
    kx2[has] = (INTR[0] * P[:, 0] / P[:, 2] + INTR[2] + rng.normal(0, 0.5, len(P))).astype("f4")
    ky2[has] = (INTR[1] * P[:, 1] / P[:, 2] + INTR[3] + rng.normal(0, 0.5, len(P))).astype("f4")
    o2[has] = o1[src[has]]
    far = has & (rng.random(n2) < 0.1)
    kx2[far] += np.float32(40.0)
    ids = np.where(rng.random(n2) < 0.8, np.arange(n2), -1).astype("i4")
    return dict(desc=np.ascontiguousarray(d2), angle=a2, kx=kx2, ky=ky2, oct=o2, src=src, ids=ids)


def invert(match12, n2):
    """vpMapPointMatches[idx2] = idx1 (ORBmatcher.cpp:251): the per-frame-feature form of match12"""
    m12 = np.asarray(match12)
    out = np.full(n2, -1, "i4")
    i1 = np.flatnonzero(m12 >= 0)
    out[m12[i1]] = i1
    assert len(np.unique(m12[i1])) == len(i1)              # a frame feature is matched at most once
    return out
