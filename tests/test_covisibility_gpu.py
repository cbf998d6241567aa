"""The device covisibility index: every output of ccm_covis_query compared exactly (all of them are integers) against the literal
walks of tests/covisibility_ref.py -- KFcounter of KeyFrame::UpdateConnections and nMPs / nRedundantObservations of
LocalMapping::KeyFrameCullingV3 -- and the culling driver against the ref's sequential loop.

The cases are built by the functions in CASES, so that a child process can run the same ones with CCM_COVIS_LDS_FEATURES=32 (the
hash in global scratch) and the parent can compare the arrays."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import covisibility_ref as R
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd import covisibility as V
from motioncheck_ccm_slam_amd.mapping import KeyFrameCulling
from motioncheck_ccm_slam_amd.tracking import MapPointTable

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U8 = np.uint8
NO_SLOT = R.NO_SLOT
CAP = 4096                                                              # slots of the small tables
CHUNK = 16                                                              # stored slots per workgroup of k_covis_weights (COVIS_CHUNK)
LIVE, BAD = _lib.MP_LIVE, _lib.MP_BAD


def rec(slots, octaves=None):
    s = np.array(slots, "i4")
    return s, (np.zeros(len(s), U8) if octaves is None else np.array(octaves, U8))


def fill(ix, records):
    for key, (s, o) in records.items():
        ix.put(key, s, o)


def live_table(ctx, capacity, slots, flags=None):
    """A table whose rows `slots` carry `flags` (default LIVE); returns (table, the flags column as the ref reads it)."""
    t = MapPointTable(capacity, ctx=ctx)
    slots = np.unique(np.asarray(slots, "i4"))
    col = np.zeros(capacity, U8)
    col[slots] = LIVE
    if flags:
        for s, f in flags.items():
            col[s] = f
    used = np.flatnonzero(col).astype("i4")
    if len(used):
        t.update(used, flags=col[used])
    return t, col


def all_slots(records):
    s = np.concatenate([r[0] for r in records.values()] + [np.zeros(0, "i4")])
    return s[(s >= 0) & (s < NO_SLOT)]


def expect(ref, ix, records, key, th_obs=3):
    """(weights row, n_mps, n_redundant, skipped) of one stored keyframe from the ref's walks"""
    row = np.zeros(ix.slots(), "i4")
    counter, _, _ = ref.update_connections(key)
    for k, w in counter.items():
        row[ix.slot(k)] = w
    n_mps, n_red = ref.counts(key, th_obs)
    skipped = sum(1 for s in records[key][0].tolist() if 0 <= s < NO_SLOT and s in ref.mp_bad)
    return row, n_mps, n_red, skipped


def check(ix, records, keys, table=None, flags=None, th_obs=3, what=3, ctx=None, ref=None):
    ref = ref if ref is not None else R.RefMap(records, flags)
    r = ix.query(keys, table=table, what=what, th_obs=th_obs, ctx=ctx)
    stored = np.zeros(ix.slots(), bool)
    for k in records:
        stored[ix.slot(k)] = True
    assert np.array_equal(r.seq >= 0, stored)
    for i, key in enumerate(keys):
        row, n_mps, n_red, skipped = expect(ref, ix, records, key, th_obs)
        if what & V.COVIS_WEIGHTS:
            assert np.array_equal(r.weights[i], row), (key, r.weights[i], row)
            assert r.weights[i][ix.slot(key)] == 0 and not r.weights[i][~stored].any()
        else:
            assert r.weights is None
        assert r.n_mps[i] == n_mps and r.skipped[i] == skipped, (key, r.n_mps[i], n_mps, r.skipped[i], skipped)
        if what & V.COVIS_REDUNDANCY:
            assert r.n_redundant[i] == n_red, (key, r.n_redundant[i], n_red)
        else:
            assert r.n_redundant is None
    return r


# ---------------------------------------------------------------- the cases (also run by the child process)

def case_lengths(rng):
    """Record lengths 0, 1, 63, 64, 65, 129, 300; a record equal to the query; one that shares nothing; slot 0 and slot CAP - 1;
    ids -1 and INT32_MAX in the query and in the records."""
    pool = rng.permutation(np.arange(1, CAP - 1)).astype("i4")
    q = np.concatenate([[0, CAP - 1], pool[:296], [-1, NO_SLOT]]).astype("i4")          # 300 features, 298 of them with a slot
    rng.shuffle(q)
    records = {0: (q, rng.integers(0, 8, 300).astype(U8))}
    records[1] = (q.copy(), rng.integers(0, 8, 300).astype(U8))                         # equal to the query
    records[2] = (pool[2000:2200].copy(), np.zeros(200, U8))                            # shares nothing
    key = 3
    for n in (0, 1, 63, 64, 65, 129, 300) * 2:
        mostly_q = q[(q >= 0) & (q < NO_SLOT)]
        if key % 2:
            s = rng.choice(mostly_q, min(n, len(mostly_q)), replace=False)
            s = np.concatenate([s, pool[3000:3000 + n - len(s)]])
        else:
            s = rng.choice(pool[:1200], n, replace=False)
        s = s.astype("i4")
        if n >= 63:
            s[5] = -1; s[17] = NO_SLOT; s[n - 1] = -7
        records[key] = (s, rng.integers(0, 8, n).astype(U8)); key += 1
    records[key] = rec([0]); key += 1
    records[key] = rec([CAP - 1, NO_SLOT, -1]); key += 1
    return records, [0, 1, 3, 4, 9, key - 1, 2]


def case_strides(k):
    """Query slots in strides of 2^k; the records hold every other one, every third one, and neighbours that are not in the query."""
    n = 40
    q = (np.arange(n, dtype="i8") << k).astype("i4")
    records = {0: (q, np.zeros(n, U8)), 1: (q[::2].copy(), np.zeros(n // 2, U8)), 2: (q[::3].copy(), np.ones(len(q[::3]), U8)),
               3: ((q[1:] - 1 if k else q[:0]).astype("i4"), np.zeros(n - 1 if k else 0, U8)), 4: (q[::-1].copy(), np.zeros(n, U8)),
               5: (q[7:9].copy(), np.zeros(2, U8))}
    return records, [0, 1, 5]


def case_powers_of_two(rng):
    """Queries with exactly 64, 65, 128 and 129 counting entries: the hash is exactly half full, and one beyond."""
    pool = rng.permutation(CAP).astype("i4")
    records = {}
    for key, n in enumerate((64, 65, 128, 129)):
        records[key] = (np.concatenate([pool[:n], [-1, NO_SLOT]]).astype("i4"), rng.integers(0, 4, n + 2).astype(U8))
    records[10] = (pool[:129][::-1].copy(), rng.integers(0, 4, 129).astype(U8))
    records[11] = (pool[60:70].copy(), np.zeros(10, U8))
    return records, [0, 1, 2, 3]


def case_redundancy():
    """Point 1: observers at octave_q + 1 (counts) and octave_q + 2 (does not): with two more exactly th_obs.  Point 2: exactly
    th_obs - 1.  Point 3: octave 255 in the query (everything is fine enough).  Point 4: octave 255 in an observer.  Point 5: nobody
    else.  Point 6: four observers, all too coarse."""
    records = {
        0: rec([1, 2, 3, 4, 5, 6], [3, 3, 255, 0, 0, 1]),
        1: rec([1, 2, 3, 4, 6], [4, 4, 255, 255, 3]),
        2: rec([1, 2, 3, 4, 6], [5, 0, 254, 1, 3]),
        3: rec([1, 3, 4, 6], [0, 0, 1, 9]),
        4: rec([1, 3, 4, 6], [2, 7, 0, 200]),
        5: rec([4], [1]),
    }
    return records, [0, 1, 2, 3, 4, 5]


def case_random(rng, n_kf=24, n_points=600, table=False):
    """A map with shared points, holes, points without a slot and, with a table, bad rows, rows that are not live and ids beyond it."""
    records = {}
    for key in range(n_kf):
        n = int(rng.integers(8, 300))
        s = rng.choice(n_points, n, replace=False).astype("i4")
        holes = rng.random(len(s))
        s[holes < 0.2] = -1
        s[holes > 0.97] = NO_SLOT
        if table:
            s[np.isin(s, [3, 4, 5, 6])] = -1
            s[:2] = [CAP + key, CAP + 1000 + key]                                       # beyond the table
            s[2:6] = [3, 4, 5, 6]                                                       # the rows the table tests flag
        records[key * 7 + 1] = (s, rng.integers(0, 8, len(s)).astype(U8))
    return records, [k * 7 + 1 for k in (0, 5, 11, 23, 2)]


CASES = [("lengths", lambda: case_lengths(np.random.default_rng(1))),
         ("powers", lambda: case_powers_of_two(np.random.default_rng(2))),
         ("redundancy", case_redundancy),
         ("random", lambda: case_random(np.random.default_rng(3)))] + \
        [("stride%d" % k, (lambda k=k: case_strides(k))) for k in range(17)]


def run_case(ctx, records, keys, th_obs=3):
    ix = V.CovisibilityIndex(1024, ctx=ctx)
    fill(ix, records)
    r = ix.query(keys, th_obs=th_obs)
    return ix, r


def child_main(path):
    """Runs every case without a table and saves the arrays: what the parent compares with its own."""
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    ctx = _lib.Context(0)
    out = {"lds_features": np.array([_lib.load().ccm_covis_lds_features()])}
    for name, build in CASES:
        records, keys = build()
        _, r = run_case(ctx, records, keys)
        out[name + ".w"] = r.weights; out[name + ".m"] = r.n_mps; out[name + ".r"] = r.n_redundant; out[name + ".s"] = r.skipped
    # with a table as well: the flags are read while the global hash is built
    records, keys = case_random(np.random.default_rng(4), table=True)
    t, _ = live_table(ctx, CAP, all_slots(records)[all_slots(records) < CAP], {3: LIVE | BAD, 4: 0, 5: BAD})
    ix = V.CovisibilityIndex(1024, ctx=ctx)
    fill(ix, records)
    r = ix.query(keys, table=t)
    out["table.w"] = r.weights; out["table.m"] = r.n_mps; out["table.r"] = r.n_redundant; out["table.s"] = r.skipped
    np.savez(path, **out)
    ctx.close()


# ---------------------------------------------------------------- tests

@pytest.mark.parametrize("name", [n for n, _ in CASES if not n.startswith("stride")])
def test_cases_match_the_ref(ctx, name):
    records, keys = dict(CASES)[name]()
    ix = V.CovisibilityIndex(1024, ctx=ctx)
    fill(ix, records)
    ref = R.RefMap(records)
    r = check(ix, records, keys, ref=ref)
    if name == "lengths":
        assert r.weights[0][ix.slot(1)] == 298 and r.weights[0][ix.slot(2)] == 0 and r.n_mps[0] == 298 and not r.skipped.any()
        assert r.weights[1][ix.slot(0)] == 298                                          # -1 and INT32_MAX never match
    if name == "redundancy":
        # point 1: octaves 4 (+1, counts), 5 (+2, does not), 0, 2 -> 3 = th_obs; point 2: 4, 0 -> 2 = th_obs - 1; point 3: 255 in the
        # query, four observers; point 4: 255 does not count, 1, 1, 0, 1 do; point 5: alone; point 6: 3, 3, 9, 200 against 1 + 1
        assert r.n_mps[0] == 6 and r.n_redundant[0] == 3
        assert check(ix, records, [0], th_obs=4, ref=ref).n_redundant[0] == 2
        assert check(ix, records, [0], th_obs=2, ref=ref).n_redundant[0] == 4
        assert check(ix, records, [0], th_obs=1, ref=ref).n_redundant[0] == 4
    # a batch equals the single queries; WEIGHTS alone, REDUNDANCY alone and both agree
    for i, key in enumerate(keys):
        one = check(ix, records, [key], ref=ref)
        assert np.array_equal(one.weights[0], r.weights[i]) and one.n_redundant[0] == r.n_redundant[i]
    w = check(ix, records, keys, what=V.COVIS_WEIGHTS, ref=ref)
    d = check(ix, records, keys, what=V.COVIS_REDUNDANCY, ref=ref)
    assert np.array_equal(w.weights, r.weights) and np.array_equal(d.n_redundant, r.n_redundant) and np.array_equal(w.n_mps, d.n_mps)


def test_stored_record_counts_around_the_chunk(ctx):
    """1, 3, 4, 5 (the waves of a workgroup), 15, 16, 17 (its chunk), 31, 32, 33 (two chunks) and 48 stored records; the query's own
    slot and the slots freed by erase give 0."""
    rng = np.random.default_rng(5)
    ix = V.CovisibilityIndex(256, ctx=ctx)
    records = {}
    for n in range(1, 49):
        key = 1000 + n
        s = rng.choice(400, int(rng.integers(1, 120)), replace=False).astype("i4")
        records[key] = (s, rng.integers(0, 6, len(s)).astype(U8))
        ix.put(key, *records[key])
        if n in (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 48):
            assert ix.slots() == n
            check(ix, records, [1001, key, 1000 + (n + 1) // 2])
    for key in (1001, 1016, 1017, 1048, 1030):                          # free slots: the first, the chunk's edges, the last
        ix.erase(key); del records[key]
    assert ix.slots() == 48 and ix.size() == 43
    r = check(ix, records, [1002, 1047, 1033])
    assert (r.seq < 0).sum() == 5
    ix.put(2000, *records[1002]); records[2000] = records[1002]         # a freed slot taken again, by a copy of a stored record
    assert ix.slots() == 48
    r = check(ix, records, [1002, 2000])
    assert r.weights[0][ix.slot(2000)] == len(records[1002][0])


@pytest.fixture(scope="module")
def stride_table(ctx):
    """One table large enough for 40 slots in strides of 2^16, its rows LIVE where any stride case puts a slot."""
    slots = np.unique(np.concatenate([all_slots(case_strides(k)[0]) for k in range(17)]))
    t, col = live_table(ctx, (40 << 16) + 1, slots)
    yield t, col
    t.close()


@pytest.mark.parametrize("k", range(17))
def test_hash_stress_strides_of_two_to_the_k(ctx, stride_table, k):
    records, keys = case_strides(k)
    ix = V.CovisibilityIndex(1024, ctx=ctx)
    fill(ix, records)
    ref = R.RefMap(records)
    r = check(ix, records, keys, ref=ref)
    assert r.weights[0][ix.slot(1)] == 20 and r.weights[0][ix.slot(4)] == 40 and r.weights[0][ix.slot(3)] == 0
    t, col = stride_table
    rt = check(ix, records, keys, table=t, flags=col)
    assert np.array_equal(rt.weights, r.weights) and not rt.skipped.any()


def test_table_flags_skip_and_count(ctx):
    rng = np.random.default_rng(4)
    records, keys = case_random(rng, table=True)
    inside = all_slots(records); inside = inside[inside < CAP]
    special = {3: LIVE | BAD, 4: 0, 5: BAD, 6: LIVE | _lib.MP_HAS_OBS}
    t, col = live_table(ctx, CAP, inside, special)
    ix = V.CovisibilityIndex(1024, ctx=ctx)
    fill(ix, records)
    r = check(ix, records, keys, table=t, flags=col)
    for i, key in enumerate(keys):
        s = records[key][0]
        want = int(np.isin(s, [3, 4, 5]).sum() + (s[(s >= 0) & (s < NO_SLOT)] >= CAP).sum())
        assert r.skipped[i] == want
    assert (r.skipped == 5).all()                                       # two ids beyond the table, a BAD row, a dead row, a BAD dead row
    # without a table the same rows count
    r0 = check(ix, records, keys)
    assert not r0.skipped.any() and (r0.n_mps == r.n_mps + r.skipped).all() and (r0.weights >= r.weights).all()
    # through a view attached from a second context
    other = _lib.Context(0)
    try:
        view = t.attach(other)
        rv = check(ix, records, keys, table=view, flags=col, ctx=other)
        for a, b in zip(rv[:5], r[:5]):
            assert np.array_equal(a, b)
        # a row that turns bad through the first handle is seen by the view's next query
        s0 = records[keys[0]][0]
        victim = int(s0[(s0 >= 7) & (s0 < CAP)][0])
        t.update(np.array([victim], "i4"), flags=np.array([LIVE | BAD], U8)); col[victim] = LIVE | BAD
        rv2 = check(ix, records, keys, table=view, flags=col, ctx=other)
        assert rv2.skipped[0] == r.skipped[0] + 1
        view.close()
    finally:
        other.close()
    t.close()


def test_pair_count_where_a_point_is_held_twice(ctx):
    """Not a state of the reference; the defined result is the number of pairs."""
    records = {1: rec([5, 5, 6, 7, -1, 8]), 2: rec([5, 9]), 3: rec([5, 5, 5, 6]), 4: rec([6, 6, 7, 7, 7]), 5: rec([10])}
    ix = V.CovisibilityIndex(64, ctx=ctx)
    fill(ix, records)
    r = ix.query([1, 3, 4])
    for i, key in enumerate([1, 3, 4]):
        want = R.pair_weights(records, key)
        for k, w in want.items():
            assert r.weights[i][ix.slot(k)] == w
        assert r.weights[i][ix.slot(key)] == 0
    assert list(r.weights[0][[ix.slot(k) for k in (2, 3, 4, 5)]]) == [2, 7, 5, 0]      # 2x1; 2x3 + 1x1; 1x2 + 1x3
    assert list(r.n_mps) == [5, 4, 5]
    # redundancy counts pairs too.  Keyframe 1: each of its two features of point 5 meets 1 + 3 features, point 6 meets 1 + 2, point 7
    # meets 3.  Keyframe 3: each of its three features of point 5 meets 2 + 1, point 6 meets 1 + 2.  Keyframe 4: 6 meets 1 + 1, 7 meets 1.
    assert list(r.n_redundant) == [4, 4, 0]


def test_arena_grows_and_is_compacted(ctx):
    rng = np.random.default_rng(6)
    ix = V.CovisibilityIndex(512, ctx=ctx)
    assert ix.arena() == (512, 0, 0)
    records = {}

    def put(key, n):
        s = rng.choice(900, n, replace=False).astype("i4")
        records[key] = (s, rng.integers(0, 8, n).astype(U8))
        ix.put(key, *records[key])

    for key in range(4):
        put(key, 100)
    check(ix, records, [0, 3])
    assert ix.arena() == (512, 400, 400)
    for key in range(4, 30):                                            # longer and longer records until it grows
        put(key, 100 + 6 * key)
    r1 = check(ix, records, [0, 3, 29])
    cap1, used1, live1 = ix.arena()
    total = sum(len(s) for s, _ in records.values())
    assert cap1 > 512 and used1 == live1 == total
    slot3 = ix.slot(3)
    put(3, 250)                                                         # a replace keeps slot and sequence number (the full arena grows again)
    r2 = check(ix, records, [0, 3, 29])
    cap_b, used_b, live_b = ix.arena()
    assert cap_b > cap1 and live_b == live1 + 150 and np.array_equal(r2.seq, r1.seq) and ix.slot(3) == slot3
    put(3, 100)                                                         # ... and, where there is room, leaves a hole behind
    r3 = check(ix, records, [0, 3, 29])
    assert ix.arena() == (cap_b, used_b + 100, live_b - 150) and np.array_equal(r3.seq, r1.seq)
    used1 = used_b + 100
    before = check(ix, records, [29, 28])
    for key in range(0, 22):                                            # more than half of the arena becomes holes
        ix.erase(key); del records[key]
    after = check(ix, records, [29, 28])
    cap2, used2, live2 = ix.arena()
    assert used2 == live2 == sum(len(s) for s, _ in records.values()) and used2 < used1 // 2 and cap2 == cap_b
    keep = [ix.slot(k) for k in records]
    assert np.array_equal(after.weights[:, keep], before.weights[:, keep])
    ix.clear()
    assert ix.slots() == 0
    records = {}
    put(77, 10); put(78, 10)
    check(ix, records, [77, 78])


def test_replacing_uploaded_records_triggers_the_compaction(ctx):
    """Holes left by `put` of present keys alone (no erase) pass half of the used arena: the next query compacts around the records
    that were not replaced and appends the replacements, in a capacity that does not change."""
    rng = np.random.default_rng(16)
    ix = V.CovisibilityIndex(512, ctx=ctx)
    records = {}

    def put(key, n):
        records[key] = (rng.choice(200, n, replace=False).astype("i4"), rng.integers(0, 8, n).astype(U8))
        ix.put(key, *records[key])

    for key in range(12):
        put(key, 30)
    before = check(ix, records, [0, 5, 11])
    assert ix.arena() == (512, 360, 360)
    for key in range(1, 9):                                             # 240 of the 360 uploaded features become holes
        put(key, 25 + key)
    after = check(ix, records, [0, 5, 11])                              # 5 was replaced; 0 and 11 were moved
    live = sum(len(s) for s, _ in records.values())
    assert ix.arena() == (512, live, live) and live == 120 + 8 * 25 + 36
    assert np.array_equal(after.seq, before.seq) and [ix.slot(k) for k in range(12)] == list(range(12))
    assert np.array_equal(after.weights[[0, 2]][:, [0, 9, 10, 11]], before.weights[[0, 2]][:, [0, 9, 10, 11]])
    put(9, 31)                                                          # one hole of 30 in 356: no compaction, the record goes to the tail
    check(ix, records, [9, 0])
    assert ix.arena() == (512, live + 31, live + 1)


def test_argument_checks(ctx):
    lib = _lib.load()
    ix = V.CovisibilityIndex(64, ctx=ctx)
    records = {k: rec([1, 2, 3, k + 10]) for k in range(5)}
    fill(ix, records)
    before = check(ix, records, [0, 1])
    q = np.array([0, 1], "i8")
    w = np.zeros((2, 8), "i4"); nm = np.zeros(2, "i4"); nr = np.zeros(2, "i4"); sk = np.zeros(2, "i4")
    res = _lib.CovisResult(3, _lib.ptr(w), _lib.ptr(nm), _lib.ptr(nr), _lib.ptr(sk), None)
    import ctypes as C

    def call(c, table, n_q, keys, what, cap, result=res):
        return lib.ccm_covis_query(c.handle, ix.handle, table, n_q, _lib.ptr(keys), what, cap, C.byref(result))

    assert call(ctx, None, 2, q, 3, 8) == 5
    assert call(ctx, None, 2, np.array([0, 99], "i8"), 3, 8) == -1 and "99" in lib.ccm_last_error(ctx.handle).decode()       # unknown key
    for what in (0, 4, 7, -1):
        assert call(ctx, None, 2, q, what, 8) == -1
    assert call(ctx, None, 2, q, 3, 4) == -4                            # CCM_E_CAPACITY: 5 slots, room for 4
    assert call(ctx, None, 0, q, 3, 0) == 0                             # n_q == 0
    assert call(ctx, None, -1, q, 3, 8) == -1
    for th in (0, -3, (1 << 20) + 1):
        bad = _lib.CovisResult(th, _lib.ptr(w), _lib.ptr(nm), _lib.ptr(nr), _lib.ptr(sk), None)
        assert call(ctx, None, 2, q, 2, 8, bad) == -1
        assert call(ctx, None, 2, q, 1, 8, bad) == 5                    # th_obs is read with REDUNDANCY only
    none = _lib.CovisResult(3, None, None, None, None, None)
    assert call(ctx, None, 2, q, 1, 8, none) == -1 and call(ctx, None, 2, q, 2, 8, none) == -1
    other = _lib.Context(0)
    try:
        t = MapPointTable(64, ctx=other)
        assert call(ctx, C.c_void_p(t.handle), 2, q, 3, 8) == -1        # a table of another context
        assert "another context" in lib.ccm_last_error(ctx.handle).decode()
        assert call(other, C.c_void_p(t.handle), 2, q, 3, 8) == 5       # ... and with its own: every row is dead, all skipped
        assert list(sk) == [4, 4] and list(nm) == [0, 0]
        t.close()
    finally:
        other.close()
    import torch
    if torch.cuda.device_count() > 1:                                   # a context on another device
        far = _lib.Context(1)
        try:
            assert call(far, None, 2, q, 3, 8) == -1 and "device" in lib.ccm_last_error(far.handle).decode()
        finally:
            far.close()
    after = check(ix, records, [0, 1])
    assert all(np.array_equal(a, b) for a, b in zip(before[:5], after[:5]))


def test_global_hash_path_equals_the_lds_path(ctx, tmp_path):
    """The same cases in a child process with CCM_COVIS_LDS_FEATURES=32: every query longer than 32 features is hashed in global
    scratch."""
    assert V.CovisibilityIndex(0, ctx=ctx).lds_features() > 300          # this process hashes every case in LDS
    path = str(tmp_path / "child.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_covisibility_gpu as T; T.child_main(%r)" % (os.path.dirname(HERE), HERE, path))
    env = dict(os.environ, CCM_COVIS_LDS_FEATURES="32")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.load(path)
    assert got["lds_features"][0] == 32
    n_global = 0
    for name, build in CASES:
        records, keys = build()
        n_global += sum(len(records[k][0]) > 32 for k in keys)
        _, r = run_case(ctx, records, keys)
        for tag, a in ((".w", r.weights), (".m", r.n_mps), (".r", r.n_redundant), (".s", r.skipped)):
            assert np.array_equal(got[name + tag], a), name + tag
    assert n_global >= 20
    records, keys = case_random(np.random.default_rng(4), table=True)
    t, col = live_table(ctx, CAP, all_slots(records)[all_slots(records) < CAP], {3: LIVE | BAD, 4: 0, 5: BAD})
    ix = V.CovisibilityIndex(1024, ctx=ctx)
    fill(ix, records)
    r = check(ix, records, keys, table=t, flags=col)
    for tag, a in ((".w", r.weights), (".m", r.n_mps), (".r", r.n_redundant), (".s", r.skipped)):
        assert np.array_equal(got["table" + tag], a), tag
    t.close()


def test_two_threads_query_while_a_third_puts_and_erases(ctx):
    """The third thread's keyframes share no point with the queried ones: whatever serial order the calls took, the queried rows are
    the ref's on the slots the test filled, and 0 on every slot the third thread may hold at that moment."""
    rng = np.random.default_rng(8)
    records, keys = case_random(rng, n_kf=30)
    ix = V.CovisibilityIndex(2048, ctx=ctx)
    fill(ix, records)
    ref = R.RefMap(records)
    n0 = ix.slots()
    want = {k: expect(ref, ix, records, k) for k in keys}
    other = _lib.Context(0)
    out, err = {}, []

    def run(name, c):
        try:
            out[name] = [ix.query([k, keys[0]], ctx=c) for k in keys * 3]
        except Exception as e:                                          # noqa: BLE001
            err.append(e)

    def churn():
        try:
            for i in range(40):
                s = (100000 + rng.choice(500, 50, replace=False)).astype("i4")
                ix.put(9000 + i % 7, s, np.zeros(50, U8))
                if i % 3 == 2:
                    ix.erase(9000 + (i - 2) % 7)
        except Exception as e:                                          # noqa: BLE001
            err.append(e)

    try:
        th = [threading.Thread(target=run, args=("a", other)), threading.Thread(target=run, args=("b", ctx)), threading.Thread(target=churn)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not err, err
        for name in ("a", "b"):
            for k, r in zip(keys * 3, out[name]):
                for i, key in enumerate((k, keys[0])):
                    row, n_mps, n_red, skipped = want[key]
                    assert np.array_equal(r.weights[i][:n0], row) and not r.weights[i][n0:].any()
                    assert (r.n_mps[i], r.n_redundant[i], r.skipped[i]) == (n_mps, n_red, skipped)
        kk, _ = ix.keys()                                               # afterwards: the queried records and whatever the third thread left
        assert set(int(x) for x in kk if x >= 0) >= set(records)
        assert ix.size() == len(records) + sum(1 for x in kk if x >= 9000)
    finally:
        other.close()


def culling_map():
    """Seven keyframes.  B's points are seen by A, C, D: redundant until A is culled.  E's points are seen by A, C, D and F, so E stays
    redundant.  A is first in the list and redundant through C and D.  P's points are seen by A, C, D and F: as redundant as A, but
    protected.  Point 50 is held by A, C and D only: culling A leaves it two observers and it turns bad (src/MapPoint.cpp:494), which
    takes one point from nMPs of C and D."""
    shared = list(range(10))                  # A, B, C, D
    e_pts = list(range(20, 30))               # A, C, D, E, F
    p_pts = list(range(30, 40))               # A, C, D, F, P
    records = {
        "A": rec(shared + e_pts + p_pts + [50]),
        "B": rec(shared),
        "C": rec(shared + e_pts + p_pts + [50] + list(range(60, 75))),
        "D": rec(shared + e_pts + p_pts + [50] + list(range(80, 95))),
        "E": rec(e_pts),
        "F": rec(e_pts + p_pts + list(range(100, 140))),
        "P": rec(p_pts),
    }
    return records


def test_culling_driver_follows_the_sequential_loop(ctx):
    names = "ABCDEFP"
    key_of = {n: 10 + i for i, n in enumerate(names)}
    records = {key_of[n]: r for n, r in culling_map().items()}
    local = [key_of[n] for n in "APBCEDF"]
    protected = {key_of["P"]}
    thres = 0.9
    ref = R.RefMap(records)
    want, log = ref.keyframe_culling(local, protected, thres)
    first = {k: R.RefMap(records).counts(k) for k in local}             # the numbers of the map before anything is culled
    stale = [k for k in local if k not in protected and first[k][1] > thres * first[k][0]]
    assert first[key_of["P"]] == (10, 10)                               # redundant, and never looked at
    assert want == [key_of["A"], key_of["E"]] and stale == [key_of["A"], key_of["B"], key_of["E"]]     # B's verdict changes
    assert dict((k, (m, r)) for k, m, r in log)[key_of["C"]] == (45, 20) and first[key_of["C"]] == (46, 30)

    t, col = live_table(ctx, CAP, all_slots(records))
    ix = V.CovisibilityIndex(1024, ctx=ctx)
    fill(ix, records)
    caller = R.RefMap(records)                                          # the caller's map: SetBadFlag stays with the caller
    culled_seen = []

    def on_cull(key):
        turned = caller.set_bad_flag(key)
        culled_seen.append((key, turned))
        if turned:
            t.update(np.array(turned, "i4"), flags=np.full(len(turned), LIVE | BAD, U8))

    got = KeyFrameCulling(ix, t, local, protected, thres, on_cull=on_cull)
    assert got == want
    assert culled_seen == [(key_of["A"], [50]), (key_of["E"], [])]
    assert ix.slot(key_of["A"]) == -1 and ix.slot(key_of["P"]) >= 0 and ix.slot(key_of["B"]) >= 0
    # the index now gives the numbers of the map after the loop
    left = [k for k in local if k not in want]
    r = ix.query(left, table=t)
    for i, k in enumerate(left):
        assert (r.n_mps[i], r.n_redundant[i]) == ref.counts(k)
    t.close()


def test_connections_on_device_weights_with_ties(ctx):
    rng = np.random.default_rng(9)
    pts = np.arange(200, dtype="i4")
    records = {100: (pts, np.zeros(200, U8))}
    shares = {7: 20, 3: 15, 12: 20, 5: 15, 9: 14, 1: 40, 30: 15, 2: 0, 8: 1}
    for key, n in shares.items():
        own = 1000 * key + np.arange(30, dtype="i4")
        records[key] = (np.concatenate([rng.choice(pts, n, replace=False), own]).astype("i4"), np.zeros(n + 30, U8))
    ix = V.CovisibilityIndex(4096, ctx=ctx)
    for key in (7, 3, 100, 12, 5, 9, 1, 30, 2, 8):
        ix.put(key, *records[key])
    for rank in (None, {k: i for i, k in enumerate((5, 30, 12, 100, 3, 1, 7, 8, 9, 2))}):
        ref = R.RefMap(records, rank=rank if rank is not None else {k: ix.slot(k) for k in records})
        _, kfs, ws = ref.update_connections(100)
        got_k, got_w = ix.connections(100, rank=rank)
        assert got_k == kfs and list(got_w) == ws
        assert ws == [40, 20, 20, 15, 15, 15]
    # nothing reaches th: the single maximum, the first among the two 20s in iteration order
    ix.erase(1); del records[1]
    ref = R.RefMap(records, rank={k: ix.slot(k) for k in records})
    _, kfs, ws = ref.update_connections(100, th=21)
    got_k, got_w = ix.connections(100, th=21)
    assert got_k == kfs == [7] and list(got_w) == ws == [20]
    got_k, got_w = ix.connections(2)                                    # a keyframe that shares nothing: the reference returns early
    assert got_k == [] and len(got_w) == 0
