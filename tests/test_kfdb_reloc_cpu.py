"""ccm_kfdb_reloc_candidates (behind ccm_kfdb_shortlist with every slot eligible and min_score = -inf) against the literal walk of
DetectRelocalizationCandidates in tests/relocalization_ref.py.  No device: the per-slot arrays the query kernel would deliver are
computed in numpy, as test_kfdb_cpu.py does.  Every expectation written out by hand uses dyadic BowVector values, so the scores are
exact: a query of 4 words of 1/4 scores an entry that moves d <= 1/4 from one of those words to another with 1 - d."""
import numpy as np
import pytest

import kfdb_ref as R
import relocalization_ref as RR
from motioncheck_ccm_slam_amd import _lib, database as D

F = np.float32


class World:
    """The same keyframes in both formulations: the inverted file with mRelocScore on the keyframes, and slots with a score array."""

    def __init__(self):
        self.ref = RR.RelocDatabase()
        self.kf = {}
        self.slot_of, self.free, self.key_at, self.seq_at, self.next_seq = {}, [], [], [], 0
        self.reloc = np.zeros(16, F)
        self.frames = 0

    def make(self, key, ids, vals):
        self.kf[key] = RR.KF(key, ids, vals)
        return self.kf[key]

    def add(self, key):
        self.ref.add(self.kf[key])
        if self.free:
            s = self.free.pop()
        else:
            s = len(self.key_at); self.key_at.append(None); self.seq_at.append(-1)
        self.slot_of[key] = s; self.key_at[s] = key; self.seq_at[s] = self.next_seq; self.next_seq += 1
        self.reloc[s] = 0                                  # what database.py and the shim do at add

    def erase(self, key):
        self.ref.erase(self.kf[key])
        s = self.slot_of.pop(key)
        self.key_at[s] = None; self.seq_at[s] = -1; self.free.append(s)

    def arrays(self, ids, vals):
        n = len(self.key_at)
        words = np.zeros(n, "i4"); first = np.full(n, -1, "i4"); score = np.zeros(n, "f8")
        for s, key in enumerate(self.key_at):
            if key is not None:
                words[s], first[s], score[s] = R.per_entry(ids, vals, self.kf[key].ids, self.kf[key].vals)
        return words, score, first, np.array(self.seq_at, "i8")

    def neighbour_slots(self, key, extra=()):
        return [self.slot_of.get(k2.key, -1) for k2 in self.kf[key].best_covis[:10]] + list(extra)

    def check(self, ids, vals, extra_neighbours=()):
        """One query in both formulations; the keyframes' mRelocScore and the array must agree afterwards on every stored entry."""
        self.frames += 1
        ref = self.ref.detect_reloc(("frame", self.frames), ids, vals)
        words, score, first, seq = self.arrays(ids, vals)
        short, mcw = D.shortlist(words, score, first, seq, np.ones(len(words), np.uint8), -np.inf, -1)
        nb = [self.neighbour_slots(self.key_at[s], extra_neighbours) for s in short]
        cand = D.reloc_candidates(words, score, seq, short, nb, self.reloc)
        got = {"min_common_words": mcw, "shortlist": [self.key_at[s] for s in short], "candidates": [self.key_at[s] for s in cand]}
        assert got == {k: ref[k] for k in got}, (got, ref)
        for key, s in self.slot_of.items():
            assert self.reloc[s].tobytes() == F(self.kf[key].mRelocScore).tobytes(), key
        return ref


Q1 = (list(range(4)), [0.25] * 4)
Q2 = (list(range(20, 24)), [0.25] * 4)
N_VEC = (list(range(4)) + [20], [0.21875] * 4 + [0.125])                  # all of Q1 (score 0.875) and one word of Q2
M_VEC = (list(range(4)) + [20], [0.125] * 4 + [0.5])                        # the same words, score 0.5 for Q1


def moved(q, d):
    v = list(q[1]); v[0] += d; v[1] -= d
    return list(q[0]), v


def two_query_world():
    """Keyframes around Q1 and Q2.  N holds the four words of Q1 and one of Q2: Q1 gates it (score 0.875), Q2 lists it (one common
    word, the gate is 3) but does not score it."""
    w = World()
    w.make(1, *moved(Q1, 0.25))                                             # S: Q1 only, score 0.75
    w.make(2, *N_VEC)                                                       # N
    w.make(3, *moved(Q2, 0.25))                                             # S2: Q2 only, score 0.75
    return w


def test_a_stale_score_of_an_ungated_neighbour_changes_the_best_keyframe():
    w = two_query_world()
    for key in (1, 2, 3):
        w.add(key)
    w.make(9, [50], [1.0]); w.add(9); w.erase(9)                            # slot 3 is free from here on
    free = 3
    assert w.seq_at[free] == -1
    w.kf[3].best_covis = [w.kf[1], w.kf[2], RR.KF(77, [20], [1.0])]         # S (no word of Q2), N, and a keyframe that is not stored
    ref = w.check(*Q1)
    assert ref["shortlist"] == [1, 2] and ref["candidates"] == [1, 2] and ref["min_common_words"] == 3
    assert list(w.reloc[:3]) == [F(0.75), F(0.875), F(0)]
    before = w.reloc.copy()
    ref = w.check(*Q2, extra_neighbours=(free, -1))
    # N is listed (word 20) but not gated: its 0.875 of the first query is added and beats S2's own 0.75; S holds a stale 0.75
    # as well but shares no word with Q2 and is ignored, as are the free slot and the -1
    assert ref["listed"] == [2, 3] and ref["shortlist"] == [3] and ref["candidates"] == [2]
    assert ref["acc"] == [F(1.625)]
    assert w.reloc[1] == before[1] and w.reloc[0] == before[0]              # neither was scored by the second query
    # the same second query in a world that never ran the first: the neighbour reads 0 and S2 stays its own best
    w2 = two_query_world()
    for key in (1, 2, 3):
        w2.add(key)
    w2.kf[3].best_covis = [w2.kf[1], w2.kf[2]]
    assert w2.check(*Q2)["candidates"] == [3]


def test_a_stale_score_lifts_an_entry_over_the_retain_line():
    def run(first_query):
        w = World()
        w.make(6, *M_VEC)                                                   # M: 0.5 for Q1, one word of Q2
        w.make(4, *Q2)                                                      # T: 1.0
        w.make(3, *moved(Q2, 0.25))                                         # U: 0.75
        for key in (6, 4, 3):
            w.add(key)
        w.kf[3].best_covis = [w.kf[6]]
        if first_query:
            assert w.check(*Q1)["candidates"] == [6]
            assert w.reloc[0] == F(0.5)
        return w.check(*Q2)
    ref = run(True)                                                         # U: 0.75 + 0.5 > 0.75 * 1.25, and stays its own best
    assert ref["shortlist"] == [4, 3] and ref["acc"] == [F(1.0), F(1.25)] and ref["candidates"] == [4, 3]
    ref = run(False)                                                        # U: 0.75 == 0.75 * 1.0 is not kept
    assert ref["acc"] == [F(1.0), F(0.75)] and ref["retain"] == F(0.75) and ref["candidates"] == [4]


def test_one_best_keyframe_reached_from_two_entries_is_kept_once():
    w = World()
    w.make(4, *Q2); w.make(3, *moved(Q2, 0.25)); w.make(5, *moved(Q2, 0.125))
    for key in (3, 5, 4):
        w.add(key)
    w.kf[3].best_covis = [w.kf[4]]; w.kf[5].best_covis = [w.kf[4]]
    ref = w.check(*Q2)
    # acc 1.75, 1.875, 1.0; retain 1.40625: T's own entry falls, the other two both name T
    assert ref["shortlist"] == [3, 5, 4] and ref["acc"] == [F(1.75), F(1.875), F(1.0)] and ref["candidates"] == [4]


def test_empty_outcomes():
    w = World()
    assert w.check(*Q1) == {"listed": [], "min_common_words": 0, "shortlist": [], "candidates": []}
    w.make(1, [40, 41], [0.5, 0.5]); w.add(1)
    assert w.check(*Q1)["listed"] == []                                     # nothing shares a word
    lib = _lib.load()
    score = np.full(4, 7, F)
    assert lib.ccm_kfdb_reloc_candidates(4, None, None, None, 0, None, None, None, None) == 0
    words = np.ones(4, "i4"); sc = np.ones(4, "f8"); seq = np.arange(4, dtype="i8"); nb = np.full((1, D.NEIGHBOURS), -1, "i4"); out = np.zeros(1, "i4")
    for bad in (4, -1):                                                     # a shortlist entry outside the slots: nothing is stored
        sl = np.array([bad], "i4")
        assert lib.ccm_kfdb_reloc_candidates(4, _lib.ptr(words), _lib.ptr(sc), _lib.ptr(seq), 1, _lib.ptr(sl), _lib.ptr(nb), _lib.ptr(score),
                                             _lib.ptr(out)) == -1
    assert (score == 7).all()
    sl = np.array([0], "i4")
    assert lib.ccm_kfdb_reloc_candidates(4, _lib.ptr(words), _lib.ptr(sc), _lib.ptr(seq), 1, _lib.ptr(sl), _lib.ptr(nb), None, _lib.ptr(out)) == -1


@pytest.mark.parametrize("m, gate", [(5, 4), (10, 8), (15, 12)])
def test_word_gate_on_an_integer_is_strict(m, gate):
    assert float(F(m) * F(0.8)) == gate
    w = World()
    q = (list(range(m)), [1.0 / m] * m)
    w.make(1, *q)
    w.make(2, list(range(gate)), [1.0 / gate] * gate)                       # words == minCommonWords: fails
    w.make(3, list(range(gate + 1)), [1.0 / (gate + 1)] * (gate + 1))       # one more: passes
    for key in (2, 3, 1):
        w.add(key)
    ref = w.check(*q)
    assert ref["min_common_words"] == gate and ref["listed"] == [2, 3, 1] and ref["shortlist"] == [3, 1]


@pytest.mark.parametrize("seed", range(4))
def test_random_query_sequences_match_the_walk(seed):
    """At most 12 slots, a small vocabulary, several queries in a row with adds and erases between them: stale scores, reused
    slots and ungated neighbours all occur; the arrays' scores follow the keyframes' through the whole sequence."""
    rng = np.random.default_rng(seed)
    w = World()
    for key in range(12):
        w.make(key, *R.random_bow(rng, int(rng.integers(1, 10)), 16))
    for key in rng.permutation(12):
        w.add(int(key))
    n_cand = 0
    for step in range(8):
        for kf in w.kf.values():
            kf.best_covis = [w.kf[int(k)] for k in rng.choice(12, int(rng.integers(0, 6)), replace=False) if int(k) != kf.key]
        n_cand += len(w.check(*R.random_bow(rng, int(rng.integers(1, 10)), 16))["candidates"])
        key = int(rng.integers(0, 12))
        if key in w.slot_of:
            w.erase(key)
            w.kf[key] = RR.KF(key, w.kf[key].ids, w.kf[key].vals)           # erased and added again: a new keyframe
            for kf in w.kf.values():
                kf.best_covis = []
            if rng.random() < 0.7:
                w.add(key)
        else:
            w.add(key)
    assert n_cand > 0 and len(w.key_at) <= 12


class HostDatabase(D.KeyFrameDatabase):
    """KeyFrameDatabase with the store kept in Python, so that its DetectRelocalizationCandidates runs without a device: the
    per-slot arrays are handed in as `result`."""

    def __init__(self):
        self.w = World()
        self.reloc_score = np.zeros(0, F)

    def __del__(self):
        pass

    def add(self, key, ids, vals):
        self.w.make(key, ids, vals); self.w.add(key)
        self._reloc_reset(key)

    def erase(self, key):
        self.w.erase(key)

    def slot(self, key):
        return self.w.slot_of.get(key, -1)

    def keys(self):
        return np.array([-1 if k is None else k for k in self.w.key_at], "i8"), np.array(self.w.seq_at, "i8")

    def result(self, q):
        words, score, first, seq = self.w.arrays(*q)
        return D.QueryResult(words, score, first, seq, -1)


def test_two_queries_through_the_database_class_with_a_slot_reused_between_them():
    db = HostDatabase()
    db.add(2, *N_VEC)                                                       # N: slot 0
    db.add(3, *moved(Q2, 0.25))                                             # S2: slot 1
    covis = {3: [2, 99]}                                                    # 99 is not stored
    assert db.DetectRelocalizationCandidates(Q1, covis, result=db.result(Q1)) == [2]
    assert list(db.reloc_score[:2]) == [F(0.875), F(0)]
    assert db.DetectRelocalizationCandidates(Q2, covis, result=db.result(Q2)) == [2]      # the stale 0.875 decides
    db.erase(2)
    db.add(2, *N_VEC)                                                       # the same slot, a new keyframe: its score is 0 again
    assert db.slot(2) == 0 and db.reloc_score[0] == 0
    assert db.DetectRelocalizationCandidates(Q2, covis, result=db.result(Q2)) == [3]
    assert db.DetectRelocalizationCandidates(Q2, lambda key: covis.get(key, ()), result=db.result(Q2)) == [3]
    assert db.DetectRelocalizationCandidates(([60], [1.0]), covis, result=db.result(([60], [1.0]))) == []
