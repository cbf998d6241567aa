"""Mirror of `cslam::KeyFrameDatabase` (src/Database.cpp) on the device: `add` / `erase` / `clear`, and the candidate queries
`DetectLoopCandidates` / `DetectMapMatchCandidates` with the `minScore` loop LoopFinder and MapMatcher run in front of them, and
`DetectRelocalizationCandidates` for a Frame that is not stored.

The device computes, per stored entry, the number of words it shares with the query, the smallest shared word and the L1 score
(one kernel launch, `ccm_kfdb_query`); the ordered rest of the reference's two functions is replayed on the host over those arrays
(`shortlist`, `candidates`: pure host functions, usable without a device).  What the reference reads from the keyframes -- the
map, the covisibility graph, `msuAssClients` -- the caller passes in as `eligible` and `neighbours`."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from ._store import _Store, _check

NEIGHBOURS = 10                                         # CCM_KFDB_NEIGHBOURS: GetBestCovisibilityKeyFrames(10)

QueryResult = collections.namedtuple("QueryResult", "words score first_word seq query_slot")


def shortlist(words, score, first_word, seq, eligible, min_score: float, query_slot: int = -1):
    """Host step A (ccm_kfdb_shortlist): (slots shortlisted, in the inverted-file walk's order; minCommonWords)."""
    lib = _lib.load()
    w = np.ascontiguousarray(words, "i4"); s = np.ascontiguousarray(score, "f8"); f = np.ascontiguousarray(first_word, "i4")
    q = np.ascontiguousarray(seq, "i8"); e = np.ascontiguousarray(eligible).astype(np.uint8)
    n = len(w)
    assert len(s) == n and len(f) == n and len(q) == n and len(e) == n
    out = np.zeros(max(n, 1), "i4"); mcw = C.c_int32(0)
    m = _check(lib.ccm_kfdb_shortlist(n, _lib.ptr(w), _lib.ptr(s), _lib.ptr(f), _lib.ptr(q), _lib.ptr(e), int(query_slot),
                                      C.c_float(min_score), n, _lib.ptr(out), C.byref(mcw)), "ccm_kfdb_shortlist")
    return out[:m].copy(), int(mcw.value)


def candidates(words, score, seq, eligible, min_score: float, min_common_words: int, short, neighbours, query_slot: int = -1):
    """Host step B (ccm_kfdb_candidates).  neighbours: [len(short), <= 10] slots, -1 for none; returns the candidate slots."""
    lib = _lib.load()
    w = np.ascontiguousarray(words, "i4"); s = np.ascontiguousarray(score, "f8"); q = np.ascontiguousarray(seq, "i8")
    e = np.ascontiguousarray(eligible).astype(np.uint8); sl = np.ascontiguousarray(short, "i4")
    nb = np.full((max(len(sl), 1), NEIGHBOURS), -1, "i4")
    for i, row in enumerate(neighbours):
        row = list(row)[:NEIGHBOURS]
        nb[i, :len(row)] = row
    out = np.zeros(max(len(sl), 1), "i4")
    m = _check(lib.ccm_kfdb_candidates(len(w), _lib.ptr(w), _lib.ptr(s), _lib.ptr(q), _lib.ptr(e), int(query_slot), C.c_float(min_score),
                                       int(min_common_words), len(sl), _lib.ptr(sl), _lib.ptr(nb), _lib.ptr(out)), "ccm_kfdb_candidates")
    return out[:m].copy()


def reloc_candidates(words, score, seq, short, neighbours, reloc_score):
    """Host step B of DetectRelocalizationCandidates (ccm_kfdb_reloc_candidates) behind `shortlist` with every slot eligible and
    min_score = -inf.  reloc_score: float32 [n_slots], mRelocScore per slot, updated in place.  Returns the candidate slots."""
    lib = _lib.load()
    w = np.ascontiguousarray(words, "i4"); s = np.ascontiguousarray(score, "f8"); q = np.ascontiguousarray(seq, "i8")
    sl = np.ascontiguousarray(short, "i4")
    assert isinstance(reloc_score, np.ndarray) and reloc_score.dtype == np.float32 and reloc_score.flags.c_contiguous and len(reloc_score) >= len(w)
    nb = np.full((max(len(sl), 1), NEIGHBOURS), -1, "i4")
    for i, row in enumerate(neighbours):
        row = list(row)[:NEIGHBOURS]
        nb[i, :len(row)] = row
    out = np.zeros(max(len(sl), 1), "i4")
    m = _check(lib.ccm_kfdb_reloc_candidates(len(w), _lib.ptr(w), _lib.ptr(s), _lib.ptr(q), len(sl), _lib.ptr(sl), _lib.ptr(nb),
                                             _lib.ptr(reloc_score), _lib.ptr(out)), "ccm_kfdb_reloc_candidates")
    return out[:m].copy()


def min_score_of(score, seq, connected_slots) -> float:
    """minScore of LoopFinder.cpp:122-139 / MapMatcher.cpp:130-147 over the connected slots (ccm_kfdb_min_score), a float32 value."""
    lib = _lib.load()
    s = np.ascontiguousarray(score, "f8"); q = np.ascontiguousarray(seq, "i8"); c = np.ascontiguousarray(connected_slots, "i4")
    return float(lib.ccm_kfdb_min_score(len(s), _lib.ptr(s), _lib.ptr(q), len(c), _lib.ptr(c)))


class KeyFrameDatabase(_Store):
    """Keys are int64 (e.g. the keyframe's idpair packed by the caller); a BowVector is (ids ascending, values)."""
    _prefix = "ccm_kfdb_"

    def __init__(self, n_words: int, initial_capacity_words: int = 1 << 20, ctx: _lib.Context | None = None):
        self.lib = _lib.load()
        self.ctx = ctx if ctx is not None else _lib.default_context(0)
        h = C.c_void_p()
        self.ctx.check(self.lib.ccm_kfdb_create(self.ctx.handle, int(n_words), int(initial_capacity_words), C.byref(h)))
        self._open(h)
        self.lds_words = self.lib.ccm_kfdb_query_lds_words()
        self.reloc_score = np.zeros(0, np.float32)                      # mRelocScore per slot, kept from one query to the next

    # ---- the store (no GPU work: the entries wait in a pending list until the next query)
    def add(self, key: int, ids, vals):
        i = np.ascontiguousarray(ids, "i4"); v = np.ascontiguousarray(vals, "f8")
        assert i.ndim == 1 and i.shape == v.shape
        _check(self.lib.ccm_kfdb_add(self.handle, int(key), len(i), _lib.ptr(i), _lib.ptr(v)),
               "ccm_kfdb_add: ids must be strictly ascending and inside the vocabulary, the key new")
        self._reloc_reset(key)

    def clear(self):
        super().clear()
        self.reloc_score = np.zeros(0, np.float32)

    def _reloc_reset(self, key: int):
        """mRelocScore of a keyframe that has just been added: 0, also in a slot another keyframe held before."""
        s = self.slot(key)
        self._reloc_room(s + 1)[s] = 0

    def _reloc_room(self, n: int) -> np.ndarray:
        if len(self.reloc_score) < n:
            self.reloc_score = np.concatenate([self.reloc_score, np.zeros(max(n, 2 * len(self.reloc_score)) - len(self.reloc_score), np.float32)])
        return self.reloc_score

    def arena(self):
        """(allocated, tail, live) words of the device arena after the last query's flush."""
        return super().arena()

    def last_timing(self):
        """Milliseconds the last query spent in (flush, kernel, download)."""
        return super().last_timing()

    # ---- queries
    def query(self, key: int | None = None, bow=None, ctx: _lib.Context | None = None) -> QueryResult:
        """The raw per-slot arrays for a stored key, or for bow = (ids, vals) of a Frame that is not stored."""
        ctx = ctx if ctx is not None else self.ctx
        assert (key is None) != (bow is None), "query a stored key or a BowVector"
        cap = self.slots() + 64                                         # (another thread may add before the query takes the mutex)
        w = np.zeros(cap, "i4"); s = np.zeros(cap, "f8"); f = np.zeros(cap, "i4"); q = np.zeros(cap, "i8")
        if key is not None:
            n = ctx.check(self.lib.ccm_kfdb_query(ctx.handle, self.handle, int(key), cap, _lib.ptr(w), _lib.ptr(s), _lib.ptr(f), _lib.ptr(q)))
            qs = self.slot(key)
        else:
            i = np.ascontiguousarray(bow[0], "i4"); v = np.ascontiguousarray(bow[1], "f8")
            assert i.ndim == 1 and i.shape == v.shape
            n = ctx.check(self.lib.ccm_kfdb_query_vector(ctx.handle, self.handle, len(i), _lib.ptr(i), _lib.ptr(v), cap, _lib.ptr(w), _lib.ptr(s),
                                                         _lib.ptr(f), _lib.ptr(q)))
            qs = -1
        return QueryResult(w[:n], s[:n], f[:n], q[:n], qs)

    def min_score(self, key: int, connected_keys, ctx: _lib.Context | None = None, result: QueryResult | None = None) -> float:
        """minScore of the query keyframe over its connected keyframes that are not bad (pass `result` to reuse a query)."""
        r = result if result is not None else self.query(key, ctx=ctx)
        return min_score_of(r.score, r.seq, [self.slot(k) for k in connected_keys])

    def _eligible(self, eligible, n):
        if isinstance(eligible, np.ndarray) and eligible.dtype in (np.bool_, np.uint8):
            assert len(eligible) == n, "an eligibility mask has one byte per slot"
            return eligible.astype(np.uint8)
        m = np.zeros(n, np.uint8)
        for k in eligible:
            s = self.slot(k)
            if 0 <= s < n:
                m[s] = 1
        return m

    def _detect(self, key, min_score, eligible, neighbours, bow, ctx, result):
        r = result if result is not None else self.query(key if bow is None else None, bow=bow, ctx=ctx)
        n = len(r.words)
        keys, _ = self.keys()
        el = self._eligible(eligible, n)
        short, mcw = shortlist(r.words, r.score, r.first_word, r.seq, el, min_score, r.query_slot)
        if len(short) == 0:
            return []
        nb = []
        for s in short:
            ks = neighbours(int(keys[s])) if callable(neighbours) else neighbours.get(int(keys[s]), ())
            nb.append([self.slot(k) for k in list(ks)[:NEIGHBOURS]])
        cand = candidates(r.words, r.score, r.seq, el, min_score, mcw, short, nb, r.query_slot)
        return [int(keys[s]) for s in cand]

    def DetectRelocalizationCandidates(self, bow, neighbours, ctx=None, result=None):
        """KeyFrameDatabase::DetectRelocalizationCandidates (:329-439) for a Frame's bow = (ids, vals): every stored entry is
        eligible and there is no minimum score.  neighbours as for DetectLoopCandidates.  mRelocScore of every slot is kept in
        self.reloc_score between queries (0 for an entry no query has scored).  Returns keys."""
        r = result if result is not None else self.query(bow=bow, ctx=ctx)
        n = len(r.words)
        keys, _ = self.keys()
        short, _ = shortlist(r.words, r.score, r.first_word, r.seq, np.ones(n, np.uint8), -np.inf, -1)
        if len(short) == 0:
            return []
        nb = []
        for s in short:
            ks = neighbours(int(keys[s])) if callable(neighbours) else neighbours.get(int(keys[s]), ())
            nb.append([self.slot(k) for k in list(ks)[:NEIGHBOURS]])
        cand = reloc_candidates(r.words, r.score, r.seq, short, nb, self._reloc_room(n))
        return [int(keys[s]) for s in cand]

    def DetectLoopCandidates(self, key: int, min_score: float, eligible, neighbours, ctx=None, result=None):
        """KeyFrameDatabase::DetectLoopCandidates (:72-202).  eligible: the keys (or a per-slot mask) of the entries that are in the
        query's map and not connected to it; neighbours: key -> GetBestCovisibilityKeyFrames(10) keys (a callable or a mapping).
        LoopFinder passes min_score = float(minScore * 0.8) (the product is a double, the parameter a float).  Returns keys."""
        return self._detect(key, min_score, eligible, neighbours, None, ctx, result)

    def DetectMapMatchCandidates(self, key: int, min_score: float, eligible, neighbours, ctx=None, result=None, bow=None):
        """KeyFrameDatabase::DetectMapMatchCandidates (:204-327).  eligible: the entries whose client is not in msuAssClients of the
        query's map.  bow = (ids, vals) queries with a BowVector that is not stored (key is then ignored)."""
        return self._detect(key, min_score, eligible, neighbours, bow, ctx, result)
