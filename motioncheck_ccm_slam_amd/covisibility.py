"""The device covisibility index (include/ccm_hot.h "Covisibility"): one light record per keyframe of a map -- the map-point table
slot and the octave of every feature -- and a batched query that gives, for any number of stored keyframes at once, the counter of
`KeyFrame::UpdateConnections` (src/KeyFrame.cpp:644-662) against every stored keyframe and the counts of
`LocalMapping::KeyFrameCullingV3` (src/Mapping.cpp:818-855).  `connections` replays the ordered rest of UpdateConnections
(:664-711) on the host and needs no device; the culling loop itself is `mapping.KeyFrameCulling`."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import COVIS_REDUNDANCY, COVIS_WEIGHTS  # noqa: F401
from ._store import _Store, _check

NO_SLOT = 2 ** 31 - 1                                   # a point without a table slot yet: it never matches anything
TH_CONNECTION = 15                                      # th of UpdateConnections, src/KeyFrame.cpp:673
TH_OBS = 3                                              # thObs of KeyFrameCullingV3, src/Mapping.cpp:815

QueryResult = collections.namedtuple("QueryResult", "weights n_mps n_redundant skipped seq query_slots")


def connections(weights, rank=None, th: int = TH_CONNECTION):
    """The ordered connected keyframes of one row of weights (ccm_covis_connections): (slots, weights), descending weight and, among
    equal weights, descending iteration position (`rank` per slot; None: the slot number).  Nothing at or above `th`: the single
    maximum, the first among equals.  No weight > 0: two empty arrays (the reference leaves the connections as they are)."""
    lib = _lib.load()
    w = np.ascontiguousarray(weights, "i4"); n = len(w)
    r = None if rank is None else np.ascontiguousarray(rank, "i4")
    assert w.ndim == 1 and (r is None or r.shape == w.shape)
    s = np.zeros(max(n, 1), "i4"); ow = np.zeros(max(n, 1), "i4")
    m = _check(lib.ccm_covis_connections(n, _lib.ptr(w), _lib.ptr(r), int(th), n, _lib.ptr(s), _lib.ptr(ow)), "ccm_covis_connections")
    return s[:m].copy(), ow[:m].copy()


class CovisibilityIndex(_Store):
    """Keys are int64 (e.g. the keyframe's idpair packed by the caller).  With ctx=None and bind=False the index is created without
    a device and belongs to the device of the first context that queries it."""
    _prefix = "ccm_covis_"

    def __init__(self, initial_capacity_features: int = 1 << 20, ctx: _lib.Context | None = None, bind: bool = True):
        self.lib = _lib.load()
        self.ctx = ctx if ctx is not None else (_lib.default_context(0) if bind else None)
        h = C.c_void_p()
        rc = self.lib.ccm_covis_create(self.ctx.handle if self.ctx else None, int(initial_capacity_features), C.byref(h))
        if self.ctx:
            self.ctx.check(rc)
        else:
            _check(rc, "ccm_covis_create")
        self._open(h)

    # ---- the store (no GPU work: the records wait in a pending list until the next query)
    def put(self, key: int, slot, octave):
        """Store or replace the record of `key`: per feature the table slot it holds (negative: none; NO_SLOT: a point without a
        slot) and its octave."""
        s = np.ascontiguousarray(slot, "i4"); o = np.ascontiguousarray(octave, np.uint8)
        assert s.ndim == 1 and s.shape == o.shape
        _check(self.lib.ccm_covis_put(self.handle, int(key), len(s), _lib.ptr(s), _lib.ptr(o)), "ccm_covis_put")

    def lds_features(self) -> int:
        """The longest query record whose hash is held in LDS (ccm_covis_lds_features)."""
        return self.lib.ccm_covis_lds_features()

    def arena(self):
        """(allocated, tail, live) features of the device arena after the last query's flush."""
        return super().arena()

    def last_timing(self):
        """Milliseconds the last query spent in (flush, kernels, download)."""
        return super().last_timing()

    # ---- the query
    def query(self, keys, table=None, what: int = COVIS_WEIGHTS | COVIS_REDUNDANCY, th_obs: int = TH_OBS,
              ctx: _lib.Context | None = None) -> QueryResult:
        """All of `keys` (stored keyframes) in one call.  table: a MapPointTable (or view) of the querying context, which supplies
        isBad(), or None.  weights [n_q, slots] (None without COVIS_WEIGHTS), n_mps / n_redundant (None without COVIS_REDUNDANCY) /
        skipped [n_q], seq [slots]."""
        ctx = ctx if ctx is not None else (table.ctx if table is not None else self.ctx)
        k = np.ascontiguousarray(keys, "i8")
        assert k.ndim == 1
        n_q = len(k)
        cap = self.slots() + 64                                         # (another thread may put before the query takes the mutex)
        w = np.zeros((max(n_q, 1), cap), "i4") if what & COVIS_WEIGHTS else None
        nm = np.zeros(max(n_q, 1), "i4"); nr = np.zeros(max(n_q, 1), "i4"); sk = np.zeros(max(n_q, 1), "i4"); sq = np.full(cap, -1, "i8")
        res = _lib.CovisResult(int(th_obs), _lib.ptr(w), _lib.ptr(nm), _lib.ptr(nr), _lib.ptr(sk), _lib.ptr(sq))
        n = ctx.check(self.lib.ccm_covis_query(ctx.handle, self.handle, C.c_void_p(table.handle) if table is not None else None, n_q,
                                               _lib.ptr(k), int(what), cap, C.byref(res)))
        if n_q == 0:
            n = self.slots()
        return QueryResult(None if w is None else w[:n_q, :n], nm[:n_q], nr[:n_q] if what & COVIS_REDUNDANCY else None, sk[:n_q], sq[:n],
                           np.array([self.slot(x) for x in k], "i4"))

    def connections(self, key: int, rank=None, th: int = TH_CONNECTION, table=None, ctx=None, result: QueryResult | None = None):
        """The front half of KeyFrame::UpdateConnections for one stored keyframe: (keys, weights) of mvpOrderedConnectedKeyFrames /
        mvOrderedWeights.  rank: key -> iteration position of the reference's std::map<kfptr, int> (None: the slot number)."""
        r = result if result is not None else self.query([key], table=table, what=COVIS_WEIGHTS, ctx=ctx)
        row = r.weights[0]
        keys, _ = self.keys()
        rk = None
        if rank is not None:
            rk = np.zeros(len(row), "i4")
            for s in range(len(row)):
                if keys[s] >= 0:
                    rk[s] = rank[int(keys[s])]
        s, w = connections(row, rk, th)
        return [int(keys[i]) for i in s], w
