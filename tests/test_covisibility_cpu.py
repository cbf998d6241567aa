"""The host half of the covisibility index, without a device: tests/covisibility_ref.py against hand-computed maps,
ccm_covis_connections against the ref's ordered lists, the bookkeeping of put / erase / clear / slot / keys on an index that is
created without a context, and the argument checks that need no context.  (The checks of ccm_covis_query that need a context --
an unknown key, a table of another context, `what` -- are in test_covisibility_gpu.py: no context exists without a device.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import covisibility_ref as R
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd import covisibility as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8 = np.uint8


def rec(slots, octaves=None):
    s = np.array(slots, "i4")
    return s, (np.zeros(len(s), U8) if octaves is None else np.array(octaves, U8))


# ---------------------------------------------------------------- the ref against hand-computed cases

def test_ref_update_connections_by_hand():
    # keyframe 1 holds points 10..13; 2 shares 10, 11; 3 shares 11, 12, 13; 4 shares nothing; 5 shares 13 only
    records = {1: rec([10, 11, -1, 12, 13]), 2: rec([11, 10, 50]), 3: rec([13, 12, 11, -1]), 4: rec([60, 61]), 5: rec([13])}
    m = R.RefMap(records)
    counter, kfs, ws = m.update_connections(1, th=15)
    assert counter == {2: 2, 3: 3, 5: 1}
    assert kfs == [3] and ws == [3]                                   # nothing reaches 15: the single maximum
    counter, kfs, ws = m.update_connections(1, th=2)
    assert kfs == [3, 2] and ws == [3, 2]
    assert m.update_connections(4) == ({}, None, None)                # early return
    # point 11 bad: it is skipped when keyframe 1 walks (KeyFrame.cpp:651)
    flags = np.ones(64, U8); flags[11] = 3
    counter, _, _ = R.RefMap(records, flags).update_connections(1)
    assert counter == {2: 1, 3: 2, 5: 1}
    # a point beyond the table and a row that is not LIVE are bad too
    flags = np.ones(13, U8); flags[10] = 0
    counter, _, _ = R.RefMap(records, flags).update_connections(1)
    assert counter == {2: 1, 3: 2}


def test_ref_ties_follow_the_pointer_order():
    records = {1: rec([1, 2, 3, 4]), 2: rec([1, 2]), 3: rec([3, 4]), 4: rec([1, 3]), 5: rec([2])}
    m = R.RefMap(records)
    _, kfs, ws = m.update_connections(1, th=2)
    assert kfs == [4, 3, 2] and ws == [2, 2, 2]                       # sort ascending by (weight, pointer), then push_front
    _, kfs, ws = m.update_connections(1, th=3)
    assert kfs == [2] and ws == [2]                                   # the first maximum in iteration order: > is strict
    m = R.RefMap(records, rank={1: 0, 2: 3, 3: 1, 4: 2, 5: 4})
    _, kfs, _ = m.update_connections(1, th=2)
    assert kfs == [2, 4, 3]
    _, kfs, _ = m.update_connections(1, th=3)
    assert kfs == [3]


def test_ref_refuses_a_point_twice_in_a_keyframe():
    with pytest.raises(ValueError):
        R.RefMap({1: rec([5, 5])})
    m = R.RefMap({1: rec([R.NO_SLOT, R.NO_SLOT, -1, 4]), 2: rec([R.NO_SLOT, 4])})      # "no slot yet" holds nothing and matches nothing
    assert m.counts(1) == (1, 0) and m.update_connections(1)[0] == {2: 1}


def test_ref_culling_counts_by_hand():
    # keyframe 1: point 10 at octave 2 seen by 2 (octave 3: counts), 3 (octave 4: too coarse), 4 (0), 5 (3) -> 3 fine observers
    #             point 11 at octave 0 seen by 2, 3 at octave 1 and 4 at octave 2 -> 2 fine observers
    #             point 12 seen by nobody else; point 13 seen by 2, 3, 4 at octave 0 -> 3
    records = {1: rec([10, 11, 12, 13, -1], [2, 0, 0, 5, 0]),
               2: rec([10, 11, 13], [3, 1, 0]), 3: rec([10, 11, 13], [4, 1, 0]), 4: rec([10, 11, 13], [0, 2, 0]), 5: rec([10], [3])}
    m = R.RefMap(records)
    assert m.counts(1) == (4, 2)
    assert m.counts(1, th_obs=2) == (4, 3)
    assert m.counts(5) == (1, 1)                                      # octaves 2, 3, 4, 0 against 3 + 1
    # Observations() > thObs: point 13 above has exactly 4 observations; point 20 has 3 and cannot be redundant at thObs = 3
    m = R.RefMap({1: rec([20]), 2: rec([20]), 3: rec([20])})
    assert m.counts(1) == (1, 0) and m.Observations(20) == 3 and m.counts(1, th_obs=2) == (1, 1)


def test_ref_culling_is_sequential():
    # B's three points are seen by A, C, D; once A is culled only two fine observers are left.  A's points are seen by B, C, D.
    pts = [1, 2, 3]
    records = {"A": rec(pts), "B": rec(pts), "C": rec(pts), "D": rec(pts)}
    m = R.RefMap(records, rank={"A": 0, "B": 1, "C": 2, "D": 3})
    assert m.counts("B") == (3, 3)
    culled, log = m.keyframe_culling(["A", "B", "C"], set(), 0.9)
    assert culled == ["A"] and log == [("A", 3, 3), ("B", 3, 0), ("C", 3, 0)]
    # with a fifth observer C still has three fine observers once B is gone; D then has two; the protected A is never looked at
    records["E"] = rec(pts)
    m = R.RefMap(records, rank={k: i for i, k in enumerate("ABCDE")})
    culled, log = m.keyframe_culling(["A", "B", "C", "D"], {"A"}, 0.9)
    assert culled == ["B", "C"] and log == [("B", 3, 3), ("C", 3, 3), ("D", 3, 0)]
    # two observers left: the point turns bad and leaves the keyframes that held it (src/MapPoint.cpp:494)
    m = R.RefMap({1: rec([7, 8]), 2: rec([7, 8]), 3: rec([7, -1])})
    assert m.set_bad_flag(1) == [7, 8] and m.mp[2] == [None, None] and m.mp[3] == [None, None]
    m = R.RefMap({1: rec([7, 8]), 2: rec([7, 8]), 3: rec([7, -1]), 4: rec([7])})
    assert m.set_bad_flag(1) == [8] and m.mp[2] == [7, None] and m.Observations(7) == 3
    assert m.set_bad_flag(4) == [7] and m.mp[2] == [None, None] and m.mp[3] == [None, None]
    assert list(m.record(2)[0]) == [-1, -1]


# ---------------------------------------------------------------- ccm_covis_connections

def ref_connections(weights, rank=None, th=15):
    """The ref's ordered lists for a keyframe whose KFcounter is `weights` per slot"""
    n = len(weights)
    rk = {s: (s if rank is None else int(rank[s])) for s in range(n)}
    rk["q"] = -1
    # a map that yields exactly these weights: point (s, j) is held by the query and by slot s
    records = {"q": rec([1000 * s + j for s in range(n) for j in range(int(weights[s]))])}
    for s in range(n):
        records[s] = rec([1000 * s + j for j in range(int(weights[s]))])
    _, kfs, ws = R.RefMap(records, rank=rk).update_connections("q", th)
    return (kfs, ws) if kfs is not None else ([], [])


@pytest.mark.parametrize("weights, rank", [
    ([3, 0, 14, 14, 2], None),                    # nothing at th: the single maximum, the first among equals
    ([3, 0, 14, 14, 2], [4, 3, 2, 1, 0]),         # ... which is slot 3 in this iteration order
    ([15, 14, 16, 15, 15, 0, 40], None),          # exactly th, exactly th - 1; equal weights in descending position
    ([15, 14, 16, 15, 15, 0, 40], [3, 6, 0, 5, 1, 2, 4]),
    ([0, 0, 0], None),                            # nothing: 0
    ([], None),
    ([1], None),
    ([20, 20, 20, 20], [2, 0, 3, 1]),
])
def test_connections_replay_the_reference_order(weights, rank):
    s, w = V.connections(weights, rank)
    kfs, ws = ref_connections(weights, rank)
    assert list(s) == kfs and list(w) == ws
    assert len(s) == len(set(s)) and all(weights[i] > 0 for i in s)


def test_connections_edges_by_hand():
    s, w = V.connections([3, 0, 14, 14, 2])
    assert list(s) == [2] and list(w) == [14]
    s, w = V.connections([15, 14, 16, 15, 15, 0, 40])
    assert list(s) == [6, 2, 4, 3, 0] and list(w) == [40, 16, 15, 15, 15]
    s, w = V.connections([15, 14, 16, 15, 15, 0, 40], rank=[3, 6, 0, 5, 1, 2, 4])
    assert list(s) == [6, 2, 3, 0, 4]
    s, w = V.connections([0, 0, 0])
    assert len(s) == 0 and len(w) == 0
    s, w = V.connections([5, 9, 9], th=9)                             # th is a parameter
    assert list(s) == [2, 1]
    lib = _lib.load()
    out = np.zeros(1, "i4"); wts = np.array([20, 20], "i4")
    assert lib.ccm_covis_connections(2, _lib.ptr(wts), None, 15, 1, _lib.ptr(out), None) == -4        # CCM_E_CAPACITY
    assert lib.ccm_covis_connections(2, None, None, 15, 2, _lib.ptr(out), None) == -1                 # CCM_E_ARG
    assert lib.ccm_covis_connections(-1, _lib.ptr(wts), None, 15, 2, _lib.ptr(out), None) == -1
    assert lib.ccm_covis_connections(0, None, None, 15, 0, None, None) == 0


def test_random_connections_match_the_ref():
    rng = np.random.default_rng(3)
    for _ in range(30):
        n = int(rng.integers(1, 12))
        weights = rng.choice([0, 1, 14, 15, 16, 30], n)
        rank = rng.permutation(n) if rng.random() < 0.5 else None
        s, w = V.connections(weights, rank)
        kfs, ws = ref_connections(weights, rank)
        assert list(s) == kfs and list(w) == ws


# ---------------------------------------------------------------- bookkeeping without a device

def test_bookkeeping_without_a_device():
    ix = V.CovisibilityIndex(64, bind=False)
    assert ix.size() == 0 and ix.slots() == 0 and ix.slot(5) == -1
    for key in (100, 200, 300):
        ix.put(key, [1, 2, 3], [0, 1, 2])
    assert [ix.slot(k) for k in (100, 200, 300)] == [0, 1, 2] and ix.size() == 3 == ix.slots()
    keys, seq = ix.keys()
    assert list(keys) == [100, 200, 300] and list(seq) == [0, 1, 2]
    ix.put(200, [7] * 10, [0] * 10)                                   # a replace keeps its slot and its sequence number
    assert ix.slot(200) == 1 and ix.size() == 3
    assert list(ix.keys()[1]) == [0, 1, 2]
    ix.put(200, [], [])                                               # ... also a second time, and down to no feature at all
    assert ix.slot(200) == 1 and list(ix.keys()[1]) == [0, 1, 2]
    ix.erase(200)
    assert ix.slot(200) == -1 and ix.size() == 2 and ix.slots() == 3
    keys, seq = ix.keys()
    assert list(keys) == [100, -1, 300] and list(seq) == [0, -1, 2]
    ix.erase(200); ix.erase(12345)                                    # unknown keys: nothing happens
    assert ix.size() == 2
    ix.put(400, [1], [0])                                             # the freed slot is taken again, with a new sequence number
    assert ix.slot(400) == 1 and list(ix.keys()[1]) == [0, 3, 2] and ix.slots() == 3
    ix.put(500, [1], [0])
    assert ix.slot(500) == 3 and ix.slots() == 4
    assert ix.arena() == (0, 0, 0)                                    # nothing has reached a device
    ix.clear()
    assert ix.size() == 0 and ix.slots() == 0 and ix.slot(100) == -1
    ix.put(100, [1], [0])
    assert ix.slot(100) == 0
    assert ix.lds_features() == _lib.load().ccm_covis_lds_features() and 0 <= ix.lds_features() <= 2048


def test_argument_checks_without_a_context():
    lib = _lib.load()
    ix = V.CovisibilityIndex(0, bind=False)
    s = np.array([1, 2], "i4"); o = np.zeros(2, U8)
    assert lib.ccm_covis_put(ix.handle, 1, -1, _lib.ptr(s), _lib.ptr(o)) == -1          # n < 0
    assert lib.ccm_covis_put(ix.handle, 1, 2, None, _lib.ptr(o)) == -1
    assert lib.ccm_covis_put(ix.handle, 1, 2, _lib.ptr(s), None) == -1
    assert lib.ccm_covis_put(None, 1, 2, _lib.ptr(s), _lib.ptr(o)) == -1
    assert ix.size() == 0 and ix.slots() == 0                                           # the index is unchanged
    assert lib.ccm_covis_put(ix.handle, 1, 0, None, None) == 0                          # an empty record is legal
    for f in (lib.ccm_covis_size, lib.ccm_covis_slots, lib.ccm_covis_clear):
        assert f(None) == -1
    assert lib.ccm_covis_erase(None, 1) == -1 and lib.ccm_covis_slot(None, 1) == -1
    k = np.zeros(1, "i8")
    ix.put(2, [1], [0])
    assert lib.ccm_covis_keys(ix.handle, 1, _lib.ptr(k), None) == -4                    # CCM_E_CAPACITY: two slots
    assert lib.ccm_covis_keys(ix.handle, 2, None, None) == -1
    res = _lib.CovisResult()
    q = np.array([1], "i8")
    assert lib.ccm_covis_query(None, ix.handle, None, 1, _lib.ptr(q), 1, 8, C.byref(res)) == -1      # no context
    h = C.c_void_p()
    assert lib.ccm_covis_create(None, -1, C.byref(h)) == -1 and not h.value
    assert lib.ccm_covis_create(None, 0, None) == -1
    lib.ccm_covis_destroy(None)                                                         # a no-op


def test_symbols_are_declared_and_exported():
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "ccm_hot.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(ccm_covis_[a-z0-9_]+)\s*\(", body))
    want = {"ccm_covis_create", "ccm_covis_destroy", "ccm_covis_put", "ccm_covis_erase", "ccm_covis_clear", "ccm_covis_size",
            "ccm_covis_slot", "ccm_covis_slots", "ccm_covis_keys", "ccm_covis_query", "ccm_covis_lds_features", "ccm_covis_arena",
            "ccm_covis_last_timing", "ccm_covis_connections"}
    assert declared == want and want <= set(_lib.SYMBOLS)
    for name in want:
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+CCM_ABI_VERSION\s+3\b", txt) and lib.ccm_abi_version() == 3 == _lib.ABI_VERSION
    assert "Covisibility" in txt and _lib.COVIS_WEIGHTS == 1 and _lib.COVIS_REDUNDANCY == 2
