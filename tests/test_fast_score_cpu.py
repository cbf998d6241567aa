"""k_fast_cells's scoring, one polarity per pass (fast_arc16_split in csrc/orb_device.h), on the CPU through ccm_debug_fast_score:
what the kernel's passes store for a pixel equals the score by its definition (fast_score16, both polarities) wherever that is
>= t_lo and > 0, and nothing (-1) elsewhere.  The definition itself is checked against a numpy restatement.  No GPU."""
import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib

T_LO = (0, 1, 7, 20, 254)


def _tap(vr, t_lo):
    vr = np.ascontiguousarray(vr, np.uint8)
    assert vr.ndim == 2 and vr.shape[1] == 17
    full = np.full(len(vr), -99, np.int32)
    split = np.full(len(vr), -99, np.int32)
    assert _lib.load().ccm_debug_fast_score(_lib.ptr(vr), len(vr), int(t_lo), _lib.ptr(full), _lib.ptr(split)) == 0
    return full, split


def _arcs(vr):
    """(brighter, darker): max over the 16 arcs of 9 contiguous ring pixels of min(ring - v), of min(v - ring)."""
    v = vr[:, :1].astype(np.int32)
    r = vr[:, 1:].astype(np.int32)
    out = []
    for e in (r - v, v - r):
        e2 = np.concatenate([e, e[:, :8]], axis=1)
        out.append(np.max([e2[:, k:k + 9].min(axis=1) for k in range(16)], axis=0))
    return out


def _flags(vr, t_lo):
    v = vr[:, 0].astype(np.int32)
    r = vr[:, 1:].astype(np.int32)
    can_b = np.minimum(np.maximum(r[:, 0], r[:, 8]), np.maximum(r[:, 4], r[:, 12])) > v + t_lo
    can_d = np.maximum(np.minimum(r[:, 0], r[:, 8]), np.minimum(r[:, 4], r[:, 12])) < v - t_lo
    return can_b, can_d


def _ring(v, values):
    return np.concatenate([[v], values]).clip(0, 255).astype(np.uint8)


def _arc_rings(t_lo):
    """A flat ring around the centre with one arc of length 8, 9, 10 or 16 at contrast t_lo - 1, t_lo, t_lo + 1, brighter and
    darker, at every rotation.  The centre is 128 where the contrast fits on both sides, else at the far end of the range."""
    rows = []
    for length in (8, 9, 10, 16):
        for c in (t_lo - 1, t_lo, t_lo + 1):
            for pol in (1, -1):
                v = 128 if abs(c) <= 127 else (0 if pol * c > 0 else 255)
                for rot in range(16):
                    ring = np.full(16, v)
                    ring[(rot + np.arange(length)) % 16] = v + pol * c
                    rows.append(_ring(v, ring))
    return np.array(rows)


def _both_flag_rings(t_lo):
    """Ring pixels 0 and 4 brighter than v + t_lo, 8 and 12 darker than v - t_lo (both compass flags hold), the rest flat;
    then the same with the 9-arc 13..5 brighter (it holds 0 and 4, not 8 and 12), and with the 9-arc 5..13 darker."""
    v, c = 128, t_lo + 5
    rows = []
    for kind in ("no_arc", "bright_arc", "dark_arc"):
        ring = np.full(16, v)
        ring[[0, 4]] = v + c
        ring[[8, 12]] = v - c
        if kind == "bright_arc":
            ring[(13 + np.arange(9)) % 16] = v + c
        if kind == "dark_arc":
            ring[5 + np.arange(9)] = v - c
        rows.append(_ring(v, ring))
    return np.array(rows)


def _saturated():
    return np.array([_ring(0, np.full(16, 255)), _ring(255, np.full(16, 0))])


@pytest.fixture(scope="module")
def random_rings():
    return np.random.default_rng(3).integers(0, 256, (200_000, 17), dtype=np.uint8)


@pytest.mark.parametrize("t_lo", T_LO)
def test_split_equals_full_where_stored(random_rings, t_lo):
    vr = np.concatenate([random_rings, _arc_rings(t_lo), _both_flag_rings(t_lo), _saturated()])
    full, split = _tap(vr, t_lo)
    ab, ad = _arcs(vr)
    assert (full == np.maximum(ab, ad) - 1).all()                      # the definition
    want = np.where((full >= t_lo) & (full > 0), full, -1)
    bad = np.flatnonzero(split != want)
    assert bad.size == 0, (t_lo, vr[bad[:5]].tolist(), full[bad[:5]].tolist(), split[bad[:5]].tolist())
    # the classes are really there: pixels stored and not stored, and (where v +- t_lo leaves room for both: 2 * t_lo < 254)
    # pixels with both compass flags that store through the brighter pass, through the darker pass, and not at all
    assert (want >= 0).any() and (want < 0).any()
    can_b, can_d = _flags(vr, t_lo)
    both = can_b & can_d
    if 2 * t_lo < 254:
        assert both.any()
        assert (both & (want >= 0) & (ab > ad)).any() and (both & (want >= 0) & (ad > ab)).any() and (both & (want < 0)).any()
    else:
        assert not both.any()
    # the lemma: a polarity whose flag is false scores below t_lo
    assert (ab[~can_b] - 1 < t_lo).all() and (ad[~can_d] - 1 < t_lo).all()
    # at most one polarity stores
    thr = max(t_lo, 1)
    assert not ((ab > thr) & (ad > thr)).any()


def test_saturated_rings_score_254():
    full, split = _tap(_saturated(), 254)
    assert full.tolist() == [254, 254] and split.tolist() == [254, 254]


def test_arguments():
    lib = _lib.load()
    assert "ccm_debug_fast_score" in _lib.SYMBOLS
    assert lib.ccm_debug_fast_score(None, 0, 7, None, None) == 0
    assert lib.ccm_debug_fast_score(None, 1, 7, None, None) == -1
    assert lib.ccm_debug_fast_score(None, -1, 7, None, None) == -1
