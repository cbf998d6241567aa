"""The device KeyFrameDatabase: ccm_kfdb_query's three per-slot arrays against a Python loop (words and first_word exactly, the
double score bit for bit: its left-to-right summation order is part of its definition), and the candidate lists of
DetectLoopCandidates / DetectMapMatchCandidates against the literal inverted-file walk of tests/kfdb_ref.py."""
import threading

import numpy as np
import pytest

import kfdb_ref as R
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.database import KeyFrameDatabase

pytestmark = pytest.mark.gpu


def expected(db, entries, q_ids, q_vals):
    """The query arrays from the Python loop; entries: key -> (ids, vals) of what is stored."""
    n = db.slots()
    words = np.zeros(n, "i4"); first = np.full(n, -1, "i4"); score = np.zeros(n, "f8"); live = np.zeros(n, bool)
    for key, (ids, vals) in entries.items():
        s = db.slot(key)
        assert 0 <= s < n and not live[s]
        live[s] = True
        words[s], first[s], score[s] = R.per_entry(q_ids, q_vals, ids, vals)
    return words, first, score, live


def check(db, entries, key=None, bow=None, ctx=None):
    r = db.query(key, bow=bow, ctx=ctx)
    q_ids, q_vals = entries[key] if key is not None else bow
    words, first, score, live = expected(db, entries, q_ids, q_vals)
    assert np.array_equal(r.words, words)
    assert np.array_equal(r.first_word, first)
    assert r.score.dtype == np.float64 and np.array_equal(r.score, score)
    assert np.array_equal(r.seq >= 0, live) and len(set(r.seq[live])) == int(live.sum())
    assert r.query_slot == (db.slot(key) if key is not None else -1)
    return r


def test_entry_lengths_and_common_words_across_chunk_edges(ctx):
    rng = np.random.default_rng(1)
    db = KeyFrameDatabase(1000, 4096, ctx=ctx)
    entries = {}
    even = np.arange(0, 258, 2, dtype="i4")                              # a 129-word entry: chunks [0, 64), [64, 128), [128, 129)
    edge = even[[0, 62, 63, 64, 65, 127, 128]]
    odd = np.sort(rng.choice(np.arange(1, 999, 2), 143, replace=False)).astype("i4")
    q_ids = np.sort(np.concatenate([edge, odd])).astype("i4")            # 150 words; it meets `even` only at the chunk edges
    q_vals = rng.uniform(0.1, 1, len(q_ids)); q_vals /= q_vals.sum()
    entries[0] = (q_ids, q_vals)                                         # an entry equal to the query
    v = rng.uniform(0.1, 1, 129); entries[1] = (even, v / v.sum())
    key = 2
    for n in (0, 1, 63, 64, 65, 129) * 3:
        if key % 2:                                                      # mostly the query's words, so that whole chunks hit
            ids = np.sort(rng.choice(q_ids, n, replace=False)).astype("i4"); vals = rng.uniform(0.1, 1, n); vals /= max(vals.sum(), 1)
        else:
            ids, vals = R.random_bow(rng, n, 1000)
        entries[key] = (ids, vals); key += 1
    entries[key] = (q_ids[:1].copy(), np.ones(1)); key += 1              # one word, the query's first
    entries[key] = (q_ids[-1:].copy(), np.ones(1)); key += 1             # one word, the query's last
    for k, (ids, vals) in entries.items():
        db.add(k, ids, vals)
    assert db.size() == len(entries) == db.slots()
    r = check(db, entries, key=0)
    # (an entry equal to the query scores the sum of its normalised values: 1 to within the rounding of that sum)
    assert r.words[db.slot(0)] == 150 and abs(r.score[db.slot(0)] - 1.0) < 1e-13 and r.words[db.slot(1)] == 7
    r2 = check(db, entries, bow=(q_ids, q_vals))                         # the same query as a Frame that is not stored
    assert np.array_equal(r.score, r2.score)
    for k in (1, 2, 3, 7):                                               # lengths 129, 0, 1 and 65 as the query
        check(db, entries, key=k)


def test_query_lengths_around_the_lds_limit_and_ids_near_2_pow_20(ctx):
    """Nothing is sized by the vocabulary: a 2^20-word vocabulary, ids up to its end.  The query is staged in LDS up to
    ccm_kfdb_query_lds_words words and searched in global memory beyond."""
    rng = np.random.default_rng(2)
    n_words = 1 << 20
    db = KeyFrameDatabase(n_words, 1024, ctx=ctx)
    lds = db.lds_words
    assert lds == _lib.load().ccm_kfdb_query_lds_words() and 64 <= lds <= 4096
    pool = np.sort(np.concatenate([rng.choice(n_words - 4096, lds + 300, replace=False), np.arange(n_words - 40, n_words)])).astype("i4")
    entries = {}
    for key in range(40):
        n = int(rng.integers(0, 200))
        ids = np.sort(rng.choice(pool, n, replace=False)).astype("i4")
        if key % 4 == 0:
            ids = np.unique(np.concatenate([ids, rng.choice(n_words, 30)])).astype("i4")
        v = rng.uniform(0.1, 1, len(ids))
        entries[key] = (ids, v / max(v.sum(), 1e-9))
    entries[40] = (np.array([n_words - 1], "i4"), np.ones(1))
    for k, (ids, vals) in entries.items():
        db.add(k, ids, vals)
    for n in (0, 1, lds - 1, lds, lds + 1, lds + 257):
        ids = np.sort(rng.choice(pool[:-1], n, replace=False)).astype("i4") if n != 1 else pool[-1:].copy()
        v = rng.uniform(0.1, 1, n)
        r = check(db, entries, bow=(ids, v / max(v.sum(), 1e-9)))
        if n == 0:
            assert not r.words.any() and (r.first_word == -1).all() and not r.score.any()
        if n == 1:
            assert r.words[db.slot(40)] == 1 and r.first_word[db.slot(40)] == n_words - 1
        if n >= lds - 1:
            assert (r.words > 64).any()
    # a stored query on each side of the limit (it is then read from the arena itself)
    for key, n in ((100, lds), (101, lds + 1)):
        ids = np.sort(rng.choice(pool, n, replace=False)).astype("i4"); v = rng.uniform(0.1, 1, n)
        entries[key] = (ids, v / v.sum())
        db.add(key, *entries[key])
    check(db, entries, key=100)
    r = check(db, entries, key=101)
    assert abs(r.score[db.slot(101)] - 1.0) < 1e-12 and r.words[db.slot(100)] > 64


def test_arena_growth_compaction_slot_reuse_and_clear(ctx):
    rng = np.random.default_rng(3)
    db = KeyFrameDatabase(1000, 512, ctx=ctx)
    assert db.arena() == (512, 0, 0)
    entries = {}

    def add(key):
        entries[key] = R.random_bow(rng, int(rng.integers(20, 60)), 300)
        db.add(key, *entries[key])

    for key in range(5):
        add(key)
    check(db, entries, key=0)                                            # fits: no growth
    cap0, used0, live0 = db.arena()
    total = sum(len(i) for i, _ in entries.values())
    assert cap0 == 512 and used0 == live0 == total
    for key in range(5, 40):
        add(key)
    check(db, entries, key=0)                                            # before ...
    r = check(db, entries, key=7)
    cap1, used1, live1 = db.arena()                                      # ... and after growth
    assert cap1 > 512 and used1 == live1 == sum(len(i) for i, _ in entries.values()) <= cap1
    for key in range(4, 30):                                             # erase 26 of 40: more than half of the arena is holes
        db.erase(key); del entries[key]
    assert db.size() == 14 and db.slots() == 40
    r = check(db, entries, key=0)
    cap2, used2, live2 = db.arena()
    assert used2 == live2 == sum(len(i) for i, _ in entries.values()) and used2 < used1 // 2 and cap2 == cap1      # compacted
    assert (r.seq < 0).sum() == 26 and not r.words[r.seq < 0].any() and (r.first_word[r.seq < 0] == -1).all()
    db.erase(12345)                                                      # unknown key: nothing happens
    for key in range(50, 60):                                            # freed slots are taken again
        add(key)
    assert db.slots() == 40 and db.size() == 24
    r = check(db, entries, key=55)
    assert r.seq.max() == 40 + 10 - 1
    db.erase(55); add(55)                                                # erased and added before any query saw it go
    db.add(70, [], []); entries[70] = (np.zeros(0, "i4"), np.zeros(0))   # an empty entry is legal
    db.erase(70); db.add(70, [], [])
    check(db, entries, key=70)
    check(db, entries, key=55)
    db.clear()
    assert db.size() == 0 and db.slots() == 0
    r = db.query(bow=entries[0])
    assert len(r.words) == 0 and len(r.score) == 0
    entries = {}
    for key in range(3):
        add(key)
    check(db, entries, key=2)


def test_argument_checks_leave_the_database_unchanged(ctx):
    rng = np.random.default_rng(4)
    db = KeyFrameDatabase(500, 64, ctx=ctx)
    entries = {k: R.random_bow(rng, 30, 500) for k in range(6)}
    for k, e in entries.items():
        db.add(k, *e)
    before = check(db, entries, key=1)
    bad = [(10, [3, 3, 5], [.3, .3, .4]),          # not strictly ascending
           (10, [5, 3], [.5, .5]),                 # descending
           (10, [1, 500], [.5, .5]),               # outside the vocabulary
           (10, [-1, 2], [.5, .5]),
           (3, [1, 2], [.5, .5])]                  # key already present
    for key, ids, vals in bad:
        with pytest.raises(_lib.CcmError) as e:
            db.add(key, ids, vals)
        assert e.value.code == -1
    assert db.size() == 6 and db.slots() == 6 and db.slot(10) == -1
    after = check(db, entries, key=1)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    with pytest.raises(_lib.CcmError) as e:
        db.query(99)                                                     # unknown query key
    assert e.value.code == -1 and "ccm_kfdb_query" in str(e.value)
    for ids, vals in (([4, 4], [.5, .5]), ([7, 500], [.5, .5])):
        with pytest.raises(_lib.CcmError) as e:
            db.query(bow=(ids, vals))
        assert e.value.code == -1 and "ccm_kfdb_query_vector" in str(e.value)
    w = np.zeros(2, "i4"); s = np.zeros(2, "f8"); f = np.zeros(2, "i4"); q = np.zeros(2, "i8")
    rc = db.lib.ccm_kfdb_query(ctx.handle, db.handle, 1, 2, _lib.ptr(w), _lib.ptr(s), _lib.ptr(f), _lib.ptr(q))
    assert rc == -4                                                      # CCM_E_CAPACITY: 6 slots, room for 2


def test_two_contexts_and_two_threads_get_the_same_arrays(ctx):
    rng = np.random.default_rng(6)
    db = KeyFrameDatabase(1000, 512, ctx=ctx)
    entries = {k: R.random_bow(rng, int(rng.integers(1, 150)), 1000) for k in range(50)}
    for k, e in entries.items():
        db.add(k, *e)
    other = _lib.Context(0)
    try:
        a = db.query(3, ctx=other)                                       # the first query, with its flush, from the second context
        b = check(db, entries, key=3, ctx=ctx)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        db.add(50, *entries[7]); entries[50] = entries[7]
        out = {}

        def run(name, c, keys):
            out[name] = [db.query(k, ctx=c) for k in keys]

        keys = [3, 50, 7, 11, 3, 50]
        th = [threading.Thread(target=run, args=("a", other, keys)), threading.Thread(target=run, args=("b", ctx, keys))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for x, y in zip(out["a"], out["b"]):
            assert all(np.array_equal(p, q) for p, q in zip(x, y))
        for k, x in zip(keys, out["a"]):
            w, f, s, _ = expected(db, entries, *entries[k])
            assert np.array_equal(x.words, w) and np.array_equal(x.first_word, f) and np.array_equal(x.score, s)
    finally:
        other.close()


def test_score_is_the_sequential_sum(ctx):
    """Inputs on which the order of the additions shows: values scaled by 1, 1e-3 or 5 before the L1 normalisation."""
    rng = np.random.default_rng(7)
    scales = (1.0, 1e-3, 5.0)
    q_ids, q_vals = R.random_bow(rng, 150, 1000, scales)
    entries = {k: R.random_bow(rng, int(rng.integers(60, 201)), 1000, scales) for k in range(64)}
    seq = [R.l1_score(q_ids, q_vals, *entries[k]) for k in range(64)]
    rev = [R.l1_score(q_ids, q_vals, *entries[k], order="reversed") for k in range(64)]
    tree = [R.l1_score(q_ids, q_vals, *entries[k], order="tree") for k in range(64)]
    n_rev = sum(a != b for a, b in zip(seq, rev)); n_tree = sum(a != b for a, b in zip(seq, tree))
    print("entries whose double score changes: reversed order %d of 64, pairwise tree %d of 64" % (n_rev, n_tree))
    assert n_rev >= 10                                                   # the inputs can tell a wrong order from the right one
    db = KeyFrameDatabase(1000, 1 << 14, ctx=ctx)
    for k, e in entries.items():
        db.add(k, *e)
    r = check(db, entries, bow=(q_ids, q_vals))
    assert np.array_equal(r.score[[db.slot(k) for k in range(64)]], np.array(seq))
    db.add(64, q_ids, q_vals); entries[64] = (q_ids, q_vals)
    check(db, entries, key=64)


def test_candidates_match_the_inverted_file_walk(ctx):
    rng = np.random.default_rng(8)
    n = 120
    db = KeyFrameDatabase(200, 2048, ctx=ctx)
    ref = R.RefDatabase()
    kf = {}
    for key in range(n):
        ids, vals = R.random_bow(rng, int(rng.integers(20, 60)), 200)
        kf[key] = R.KF(key, ids, vals, map_id=int(rng.random() < 0.2), client=int(rng.integers(0, 4)))
    order = [int(k) for k in rng.permutation(n)]
    for key in order:
        db.add(key, kf[key].ids, kf[key].vals); ref.add(kf[key])
    for key in order[:30]:                                               # some leave, half of them come back (to the end of the lists)
        db.erase(key); ref.erase(kf[key])
    stored = set(order[30:])
    for key in order[:15]:
        db.add(key, kf[key].ids, kf[key].vals); ref.add(kf[key]); stored.add(key)
    for k in kf.values():
        k.best_covis = [kf[int(j)] for j in rng.choice(n, int(rng.integers(0, 11)), replace=False) if int(j) != k.key]
    neighbours = lambda key: [k2.key for k2 in kf[key].best_covis]
    n_cand = 0
    for i, key in enumerate(sorted(stored)[:16]):
        q = kf[key]
        q.connected = {int(j) for j in rng.choice(n, 12, replace=False)} - {key}
        res = db.query(key)
        ms = db.min_score(key, [j for j in q.connected if j in stored], result=res)
        assert np.float32(ms) == R.min_score(q, [kf[j] for j in q.connected if j in stored])
        if i % 2 == 0:
            th = float(np.float32(ms * 0.8))                              # LoopFinder.cpp:142: a double product into a float parameter
            in_map = {j for j in kf if kf[j].map_id == q.map_id}
            want = ref.detect_loop(q, th, in_map)["candidates"]
            got = db.DetectLoopCandidates(key, th, [j for j in in_map if j != key and j not in q.connected], neighbours, result=res)
        else:
            th = float(np.float32(ms)) * 0.5
            th = float(np.float32(th))
            ass = {q.client}
            want = ref.detect_map_match(q, th, ass)["candidates"]
            el = np.zeros(db.slots(), bool)
            for j in stored:
                el[db.slot(j)] = kf[j].client not in ass
            got = db.DetectMapMatchCandidates(key, th, el, {j: neighbours(j) for j in kf})
        assert got == want
        n_cand += len(want)
    assert n_cand >= 8
