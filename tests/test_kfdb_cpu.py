"""The host half of the KeyFrameDatabase (ccm_kfdb_shortlist, ccm_kfdb_candidates, ccm_kfdb_min_score) against the literal
inverted-file walk of tests/kfdb_ref.py.  No device: the per-slot arrays the kernel would deliver are computed here in numpy and
a Python loop, the two host functions replay the ordered part of DetectLoopCandidates / DetectMapMatchCandidates over them."""
import numpy as np
import pytest

import kfdb_ref as R
from motioncheck_ccm_slam_amd import _lib, database as D

F = np.float32


class World:
    """The same keyframes in both formulations: the reference's inverted file, and slots with sequence numbers."""

    def __init__(self):
        self.ref = R.RefDatabase()
        self.kf = {}                       # key -> R.KF (every keyframe, stored or not)
        self.slot_of, self.free, self.key_at, self.seq_at, self.next_seq = {}, [], [], [], 0

    def make(self, key, ids, vals, map_id=0, client=0):
        self.kf[key] = R.KF(key, ids, vals, map_id, client)
        return self.kf[key]

    def add(self, key):
        self.ref.add(self.kf[key])
        if self.free:
            s = self.free.pop()
        else:
            s = len(self.key_at); self.key_at.append(None); self.seq_at.append(-1)
        self.slot_of[key] = s; self.key_at[s] = key; self.seq_at[s] = self.next_seq; self.next_seq += 1

    def erase(self, key):
        self.ref.erase(self.kf[key])
        s = self.slot_of.pop(key)
        self.key_at[s] = None; self.seq_at[s] = -1; self.free.append(s)

    def arrays(self, q):
        n = len(self.key_at)
        words = np.zeros(n, "i4"); first = np.full(n, -1, "i4"); score = np.zeros(n, "f8")
        for s, key in enumerate(self.key_at):
            if key is not None:
                words[s], first[s], score[s] = R.per_entry(q.ids, q.vals, self.kf[key].ids, self.kf[key].vals)
        return words, score, first, np.array(self.seq_at, "i8")

    def detect(self, q, min_score, eligible_keys):
        """Both host steps over the restated arrays; returns the same dictionary as RefDatabase._finish, in keys."""
        words, score, first, seq = self.arrays(q)
        el = np.zeros(len(words), np.uint8)
        for k in eligible_keys:
            if k in self.slot_of:
                el[self.slot_of[k]] = 1
        qs = self.slot_of.get(q.key, -1)
        short, mcw = D.shortlist(words, score, first, seq, el, min_score, qs)
        nb = [[self.slot_of.get(k2.key, -1) for k2 in self.kf[self.key_at[s]].best_covis[:10]] for s in short]
        cand = D.candidates(words, score, seq, el, min_score, mcw, short, nb, qs) if len(short) else []
        return {"min_common_words": mcw, "shortlist": [self.key_at[s] for s in short], "candidates": [self.key_at[s] for s in cand]}

    def loop_eligible(self, q):
        return [k for k, kf in self.kf.items() if kf.map_id == q.map_id and k != q.key and k not in q.connected]

    def check_loop(self, q, min_score):
        ref = self.ref.detect_loop(q, min_score, {k for k, kf in self.kf.items() if kf.map_id == q.map_id})
        got = self.detect(q, min_score, self.loop_eligible(q))
        assert got == {k: ref[k] for k in got}, (got, ref)
        return ref

    def check_map_match(self, q, min_score, ass_clients):
        ref = self.ref.detect_map_match(q, min_score, ass_clients)
        got = self.detect(q, min_score, [k for k, kf in self.kf.items() if kf.client not in ass_clients])
        assert got == {k: ref[k] for k in got}, (got, ref)
        return ref


def _vec(ids, vals):
    v = np.asarray(vals, "f8")
    return list(ids), list(v / np.abs(v).sum())


def test_reference_score_is_the_host_l1_score():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    for n1, n2 in ((0, 5), (1, 1), (40, 55), (150, 200), (300, 7)):
        i1, v1 = R.random_bow(rng, n1, 400, (1.0, 1e-3, 5.0)); i2, v2 = R.random_bow(rng, n2, 400, (1.0, 1e-3, 5.0))
        got = lib.ccm_bow_score_l1(n1, _lib.ptr(i1), _lib.ptr(v1), n2, _lib.ptr(i2), _lib.ptr(v2))
        assert got == R.l1_score(i1, v1, i2, v2)                     # bit for bit (-0.0 == 0.0 for no common word)


@pytest.mark.parametrize("seed", range(6))
def test_random_worlds_match_the_inverted_file_walk(seed):
    """Small vocabulary, short vectors: many entries meet the walk at the same first word, so the add order decides; keys are
    added in shuffled order, some are erased and added again, some are connected to the query or belong to another map."""
    rng = np.random.default_rng(seed)
    w = World()
    n = 40
    for key in range(n):
        ids, vals = R.random_bow(rng, int(rng.integers(0, 14)), 30)
        w.make(key, ids, vals, map_id=int(rng.random() < 0.15), client=int(rng.integers(0, 3)))
    for key in rng.permutation(n):
        w.add(int(key))
    for key in rng.choice(n, 8, replace=False):
        w.erase(int(key))
        if rng.random() < 0.6:
            w.add(int(key))
    stored = [w.kf[k] for k in w.slot_of]
    for kf in w.kf.values():
        kf.best_covis = [w.kf[int(k)] for k in rng.choice(n, int(rng.integers(0, 13)), replace=False) if int(k) != kf.key]
    n_found = 0
    for i, q in enumerate(stored[:12]):
        q.connected = {int(k) for k in rng.choice(n, 5, replace=False)}
        ms = float(F(rng.choice([0.0, 0.05, 0.15, 0.3])))
        ref = w.check_loop(q, ms) if i % 2 == 0 else w.check_map_match(q, ms, {q.client})
        n_found += len(ref["candidates"])
    assert n_found > 0
    # a query that is not stored (a Frame): nothing in the database is "itself"
    q = w.make(1000, *R.random_bow(rng, 12, 30), client=7)
    w.check_map_match(q, 0.05, {7})


def test_ties_in_first_word_follow_the_add_order_not_the_key_order():
    w = World()
    q = w.make(100, *_vec([3, 4, 5], [1, 1, 1]))
    for key, vals in ((7, [1, 2, 1]), (2, [2, 1, 1]), (9, [1, 1, 2]), (1, [3, 1, 1])):
        w.make(key, *_vec([3, 4, 5], vals))
    for key in (7, 2, 9, 1):
        w.add(key)
    w.add(100)
    ref = w.check_loop(q, 0.0)
    assert ref["shortlist"] == [7, 2, 9, 1] and ref["listed"] == [7, 2, 9, 1]


def test_an_entry_erased_and_added_again_moves_to_the_end_of_its_lists():
    w = World()
    q = w.make(100, *_vec([0, 1], [1, 1]))
    for key in (1, 2, 3):
        w.make(key, *_vec([0, 1], [1, key + 1]))
        w.add(key)
    assert w.check_map_match(q, 0.0, {9})["shortlist"] == [1, 2, 3]
    w.erase(1); w.add(1)                                             # takes its old slot back, with a new sequence number
    assert w.slot_of[1] == 0
    q2 = w.make(101, *_vec([0, 1], [1, 1]))
    assert w.check_map_match(q2, 0.0, {9})["shortlist"] == [2, 3, 1]


@pytest.mark.parametrize("m, gate", [(5, 4), (10, 8), (15, 12), (23, 18), (64, 51)])
def test_word_gate_equality_fails(m, gate):
    assert int(F(m) * F(0.8)) == gate
    w = World()
    q = w.make(100, *_vec(range(m), np.ones(m)))
    w.make(1, *_vec(range(m), np.ones(m)))                           # maxCommonWords = m
    w.make(2, *_vec(range(gate), np.ones(gate)))                     # words == minCommonWords: fails
    w.make(3, *_vec(range(gate + 1), np.ones(gate + 1)))             # one more: passes
    for key in (2, 3, 1):
        w.add(key)
    ref = w.check_loop(q, 0.0)
    assert ref["min_common_words"] == gate and ref["shortlist"] == [3, 1] and ref["listed"] == [2, 3, 1]


def test_score_equal_to_min_score_passes_and_acc_equal_to_retain_fails():
    w = World()
    q = w.make(100, [0, 1], [0.5, 0.5])
    w.make(1, [0, 1], [0.5, 0.5])                                    # score 1.0 exactly
    w.make(2, [0, 1], [0.25, 0.75])                                  # score 0.75 exactly
    w.make(3, [0, 1], [0.25 + 2.0 ** -20, 0.75 - 2.0 ** -20])        # score 0.75 + 2^-20, a float32 value
    for key in (1, 2, 3):
        w.add(key)
    words, score, first, seq = w.arrays(q)
    assert list(score) == [1.0, 0.75, 0.75 + 2.0 ** -20]
    # min_score == (float)score of entry 2: it is shortlisted; acc == retain = 0.75f * 1.0: it is not a candidate
    ref = w.check_loop(q, 0.75)
    assert ref["shortlist"] == [1, 2, 3] and ref["candidates"] == [1, 3]
    # one float above: entry 2 is not even shortlisted
    q2 = w.make(101, [0, 1], [0.5, 0.5])
    assert w.check_loop(q2, float(np.nextafter(F(0.75), F(1))))["shortlist"] == [1, 3]


def test_neighbour_handling():
    """Query: 10 words of 0.1; an entry that moves d from one word to another scores 1 - d.  minCommonWords = 8."""
    def moved(d):
        v = np.full(10, 0.1); v[0] += d; v[1] -= d
        return list(range(10)), list(v)
    w = World()
    q = w.make(100, *moved(0.0))
    for key, d in ((1, 0.05), (2, 0.08), (3, 0.06), (4, 0.07)):                         # shortlisted entries S1 .. S4
        w.make(key, *moved(d))
    w.make(10, *moved(0.0))                                                             # N1: score 1.0 but connected to the query
    w.make(11, list(range(8)) + [10, 11], [0.1] * 10)                                   # N2: 8 common words = the gate: ungated
    w.make(12, *moved(0.0))                                                             # N3: score 1.0, eligible and gated
    w.make(13, *moved(0.05))                                                            # N4: equal to S1's score: no replacement
    w.make(14, *moved(0.0))                                                             # never stored: slot -1
    for key in (1, 2, 3, 4, 10, 11, 12, 13):
        w.add(key)
    q.connected = {10}
    w.kf[1].best_covis = [w.kf[k] for k in (10, 14, 13)]        # acc 0.95 + 0.95; N1 counted would make it 2.9 and bestKF 10
    w.kf[2].best_covis = [w.kf[k] for k in (11, 14)]            # acc 0.92; N2 counted would lift it over retain
    w.kf[3].best_covis = [w.kf[k] for k in (12,)]               # acc 1.94 = the best, bestKF N3
    w.kf[4].best_covis = [w.kf[k] for k in (12,)]               # acc 1.93, bestKF N3 again
    ref = w.check_loop(q, 0.5)
    assert ref["min_common_words"] == 8 and ref["shortlist"] == [1, 2, 3, 4, 12, 13]
    # retain = 0.75 * 1.94: S1 stays itself (N4 is not strictly greater), S2 falls, S3 and S4 both name N3 (listed once),
    # N3 and N4 on their own (1.0, 0.95) fall
    assert ref["candidates"] == [1, 12]


def test_empty_outcomes():
    w = World()
    q = w.make(100, *_vec([0, 1, 2], [1, 1, 1]))
    assert w.check_loop(q, 0.0) == {"listed": [], "min_common_words": 0, "shortlist": [], "candidates": []}      # empty database
    w.make(1, *_vec([5, 6], [1, 1])); w.add(1)
    assert w.check_loop(q, 0.0)["listed"] == []                                         # nothing shares a word
    w.make(2, *_vec([2, 6], [1, 9])); w.add(2)
    ref = w.check_loop(q, 0.9)                                                          # listed, but below min_score
    assert ref["listed"] == [2] and ref["shortlist"] == [] and ref["min_common_words"] == 0
    w.make(3, *_vec([0, 1, 2], [1, 1, 1]), map_id=1); w.add(3)
    q2 = w.make(101, *_vec([0, 1, 2], [1, 1, 1]))
    assert w.check_loop(q2, 0.9)["listed"] == [2]                                       # the perfect match is in another map
    lib = _lib.load()
    mcw = np.zeros(1, "i4")
    assert lib.ccm_kfdb_shortlist(0, None, None, None, None, None, -1, F(0), 0, None, _lib.ptr(mcw)) == 0
    assert lib.ccm_kfdb_candidates(0, None, None, None, None, -1, F(0), 0, 0, None, None, None) == 0
    assert lib.ccm_kfdb_shortlist(3, None, None, None, None, None, -1, F(0), 0, None, _lib.ptr(mcw)) == -1       # CCM_E_ARG


def test_min_score_over_connected_slots():
    rng = np.random.default_rng(11)
    w = World()
    for key in range(12):
        w.make(key, *R.random_bow(rng, 20, 40)); w.add(key)
    w.erase(4)
    q = w.kf[0]
    words, score, first, seq = w.arrays(q)
    connected = [2, 5, 9, 4, 77]                                                        # 4 is erased, 77 was never stored
    got = D.min_score_of(score, seq, [w.slot_of.get(k, -1) for k in connected] + [4])   # (and slot 4 is free)
    assert F(got) == R.min_score(q, [w.kf[k] for k in (2, 5, 9)]) and got < 1.0
    assert D.min_score_of(score, seq, []) == 1.0
