"""What `KeyFrameDatabase` and `CovisibilityIndex` share: a handle of the keyed record store (csrc/record_store.h) behind the C entry
points `<prefix>erase` ... `<prefix>last_timing`.  None of it does GPU work: records wait in a pending list until the next query."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def _check(rc: int, what: str) -> int:
    if rc < 0:
        raise _lib.CcmError(rc, what)
    return rc


class _Store:
    _prefix = ""                                            # "ccm_kfdb_" or "ccm_covis_"

    def _open(self, handle):
        """The subclass has created `handle` through self.lib: the store's entry points are looked up once, as self._erase ..."""
        for name in ("destroy", "erase", "clear", "size", "slots", "slot", "keys", "arena", "last_timing"):
            setattr(self, "_" + name, getattr(self.lib, self._prefix + name))
        self.handle = handle

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self._destroy(h); self.handle = None

    def erase(self, key: int):
        _check(self._erase(self.handle, int(key)), self._prefix + "erase")

    def clear(self):
        _check(self._clear(self.handle), self._prefix + "clear")

    def size(self) -> int:
        return self._size(self.handle)

    def slots(self) -> int:
        return self._slots(self.handle)

    def slot(self, key: int) -> int:
        return self._slot(self.handle, int(key))

    def keys(self):
        """(key per slot, -1 for a free slot; sequence number per slot)."""
        n = self.slots()
        k = np.zeros(max(n, 1), "i8"); q = np.zeros(max(n, 1), "i8")
        m = _check(self._keys(self.handle, len(k), _lib.ptr(k), _lib.ptr(q)), self._prefix + "keys")
        return k[:m], q[:m]

    def arena(self):
        a = (C.c_int64 * 3)()
        _check(self._arena(self.handle, C.byref(a, 0), C.byref(a, 8), C.byref(a, 16)), self._prefix + "arena")
        return int(a[0]), int(a[1]), int(a[2])

    def last_timing(self):
        t = np.zeros(3, "f8")
        _check(self._last_timing(self.handle, _lib.ptr(t)), self._prefix + "last_timing")
        return tuple(float(x) for x in t)
