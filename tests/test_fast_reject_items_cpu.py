"""The items of k_fast_cells's rejection test (fc_item_* in csrc/orb_device.h), on the CPU through ccm_debug_fc_items, which runs
the functions the kernel runs: wave w takes runs w, w + 4, ... of 64 items, an item is one dword dw_lo..dw_hi of a row 3..bh-4 of
the band's tile, and a lane steps from run to run without a multiply.  For every band geometry of the 752 x 480 x 8-level plan, of
the shapes of tests/test_fast_reject_items_gpu.py and of a sweep over pitch, rows and dword range: every item exactly once and
nothing else, pos0 = row * pitch + 4 * dword below 2^15, ceil(items / 64) runs, run counts of the waves at most one apart,
nothing for bh <= 6."""
import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib

import fc_band_plan_ref as plan

CAP = 65 * 64                                  # rows x dwords of the largest tile


def _items(g, cap=CAP):
    out = np.full((cap, 6), -1, np.int32)
    n = _lib.load().ccm_debug_fc_items(*[int(v) for v in g], _lib.ptr(out), cap)
    assert 0 <= n <= cap, (g, n)
    return out[:n]


def _check(g):
    pitch, bh, dw_lo, dw_hi = g
    n_dw = max(dw_hi - dw_lo + 1, 0)
    items = max(bh - 6, 0) * n_dw
    o = _items(g)
    assert len(o) == items, g
    if items == 0:
        return 0
    run, wave, lane, row, dw, pos0 = o.T
    # every (row, dword) of the detection range exactly once, nothing outside
    assert row.min() >= 3 and row.max() <= bh - 4 and dw.min() >= dw_lo and dw.max() <= dw_hi, g
    key = (row - 3) * n_dw + (dw - dw_lo)
    assert (np.sort(key) == np.arange(items)).all(), g
    assert (pos0 == row * pitch + 4 * dw).all() and pos0.max() < (1 << 15), g
    # run R is items 64 R .. 64 R + 63 in lane order, on wave R % 4; the runs come in order
    assert (key == 64 * run + lane).all() and (wave == run % 4).all() and (np.diff(run) >= 0).all(), g
    assert lane.min() >= 0 and lane.max() <= 63, g
    nruns = -(-items // 64)
    assert run.max() + 1 == nruns and len(np.unique(run)) == nruns, g
    per_wave = np.bincount(np.unique(run) % 4, minlength=4)
    assert per_wave.max() - per_wave.min() <= 1 and per_wave.tolist() == plan.wave_runs(g), g
    return nruns


GPU_SHAPES = [(182, 96, 2), (230, 80, 1), (100, 64, 1)]


def test_bench_plan():
    """752 x 480, 8 levels: 263 bands of 29 geometries, 3791 runs per frame (4292 over every dword of the tile), 979 on the
    busiest wave."""
    bands = plan.bands(752, 480, 8)
    geo = plan.geometries(752, 480, 8)
    assert len(bands) == 263 and len(geo) == 29
    nruns = {g: _check(g) for g in geo}
    key = lambda b: (b["pitch"], b["bh"], b["dw_lo"], b["dw_hi"])
    assert sum(nruns[key(b)] for b in bands) == 3791
    assert sum(plan.wave_runs(key(b))[0] for b in bands) == 979
    assert nruns[(144, 38, 1, 31)] == 16 and plan.wave_runs((144, 38, 1, 31)) == [4, 4, 4, 4]      # the dominant band


@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_gpu_test_shapes(shape):
    geo = plan.geometries(*shape)
    assert geo
    for g in geo:
        _check(g)


def test_named_bands():
    """The bands the GPU tests are built on."""
    assert (48, 38, 1, 7) in plan.geometries(182, 96, 2) and _check((48, 38, 1, 7)) == 4          # 7 detection dwords of 12
    assert _check((144, 38, 1, 31)) == 16 and _check((128, 48, 1, 30)) == 20
    assert {(g[2]) for g in plan.geometries(230, 80, 1)} == {1, 2}
    assert plan.geometries(100, 64, 1) == [(80, 32, 1, 17)] and plan.wave_runs((80, 32, 1, 17)) == [2, 2, 2, 1]


@pytest.mark.parametrize("dw_lo", [1, 2])
def test_sweep(dw_lo):
    seen = set()
    for pitch in range(16, 257, 16):
        for bh in (7, 8, 15, 37, 38, 65):
            for dw_hi in range(dw_lo, pitch // 4 - 1):
                _check((pitch, bh, dw_lo, dw_hi))
                n_dw, items = dw_hi - dw_lo + 1, (bh - 6) * (dw_hi - dw_lo + 1)
                seen |= {("n_dw", n_dw)} if n_dw in (1, 7) else set()
                seen |= {"n_dw > 64"} if n_dw > 64 else set()
                seen |= {"< 64"} if items < 64 else set()
                seen |= {"% 64"} if items % 64 == 0 else set()
                seen |= {"% 256"} if items % 256 == 0 else set()
    assert {("n_dw", 1), ("n_dw", 7), "< 64", "% 64", "% 256"} <= seen


def test_more_dwords_than_a_run():
    """n_dw > 64 needs a pitch above 256, which no band has: the tap refuses it, and the widest row (62 dwords) is in the sweep."""
    assert _lib.load().ccm_debug_fc_items(272, 38, 1, 66, None, 0) == -1
    assert _check((256, 65, 1, 62)) == -(-59 * 62 // 64)


@pytest.mark.parametrize("bh", [0, 1, 6])
def test_no_rows(bh):
    for g in plan.geometries(752, 480, 8):
        assert len(_items((g[0], bh, g[2], g[3]))) == 0


def test_tap_arguments():
    lib = _lib.load()
    assert "ccm_debug_fc_items" in _lib.SYMBOLS
    assert lib.ccm_debug_fc_items(144, 38, 1, 31, None, 0) == 992            # the count alone
    assert lib.ccm_debug_fc_items(144, 38, 2, 1, None, 0) == 0               # no detection dword
    for bad in ((144, 38, 0, 31), (144, 38, 1, 35), (12, 38, 1, 1), (146, 38, 1, 31), (144, 66, 1, 31), (144, -1, 1, 31)):
        assert lib.ccm_debug_fc_items(*bad, None, 0) == -1, bad
    out = np.zeros((4, 6), np.int32)
    assert lib.ccm_debug_fc_items(144, 38, 1, 31, _lib.ptr(out), 4) == 992 and out[3].tolist() == [0, 0, 3, 3, 4, 3 * 144 + 16]
    assert lib.ccm_debug_fc_items(144, 38, 1, 31, None, 4) == -1
