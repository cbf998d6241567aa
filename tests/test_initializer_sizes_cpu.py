"""The inputs of tests/test_initializer_sizes_gpu.py, checked without a device: the conditions the scenes must meet in the float64
reference alone, and csrc/init_math.h on the host across two tiles of matches."""
import os
import subprocess

import numpy as np

import initializer_ref as ref
import initializer_sizes as sz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_size_cases_meet_their_conditions_in_the_float64_reference():
    """Ambiguous pairs <= 1e-3 of all pairs, degenerate sets <= 2 %; the best homography of the 2049-match plane scene and the best
    fundamental matrix of the 2049-match general scene hold more than 1024 inliers, in all three tiles; at N = 1025 the best
    fundamental matrix has the lone match of the second tile as an inlier."""
    pairs = amb_n = deg_n = sets_n = 0
    for (n, share, kind, its), (p, d) in zip(sz.SIZE_CASES, sz.make_size_cases()):
        first, second, m = ref.matches_of(p)
        assert len(first) == n and d.shape == (its, 8)
        sets = ref.sample_sets(n, d)
        assert not p["wrong"][sets[:sz.PLANTED]].any() and sets[0, 0] == n - 1
        ev = ref.evaluate(p, sets)
        amb_h, amb_f = ref.ambiguous_pairs(ev)
        pairs += amb_h.size + amb_f.size; amb_n += int(amb_h.sum() + amb_f.sum()); sets_n += 2 * its
        deg_n += int((ev["gap_h"] < 1e-4).sum() + (ev["gap_f"] < 1e-4).sum())
        SH, SF, bh, bf, model = ref.select(ev["score_h"], ev["score_f"])
        best = ev["inlier_h"][bh] if kind == "plane" else ev["inlier_f"][bf]
        print("N = %d, %s: model %d, inliers of the best %s mask %d, tiles %s" % (n, kind, model, "H" if kind == "plane" else "F", best.sum(), sz.tiles_populated(best)))
        assert model == (0 if kind == "plane" else 1) and all(sz.tiles_populated(best))
        if n == 2049:
            assert best.sum() > sz.TILE
    print("ambiguous pairs %d of %d (%.4f %%), degenerate sets %d of %d (%.2f %%)" % (amb_n, pairs, 100.0 * amb_n / pairs, deg_n, sets_n, 100.0 * deg_n / sets_n))
    assert pairs == 161844 and sets_n == 106
    assert amb_n <= 1e-3 * pairs and deg_n <= 0.02 * sets_n


def test_hypothesis_math_header_past_one_tile(tmp_path):
    """tests/support/init_math_check.cpp (csrc/init_math.h on the host, the score as 64 per-lane sums in match order) on the 2049-match
    plane scene: ref.check32_h / _f fed its matrices reproduce its flags bit for bit and its scores within N 2^-20 max(score, 1)."""
    exe = str(tmp_path / "init_math_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "support", "init_math_check.cpp"), "-o", exe])
    p, d = sz.make_size_cases()[sz.PLANE_2049]
    first, second, m = ref.matches_of(p)
    n, its = len(first), len(d)
    sets = ref.sample_sets(n, d)
    T1, T2 = ref._normalize32(p["kp1"]), ref._normalize32(p["kp2"])
    blob = (np.array([n, its], "i4").tobytes() + T1.tobytes() + T2.tobytes() + np.float32(1.0).tobytes() + m.astype("f4").tobytes() + sets.astype("i4").tobytes())
    out = subprocess.run([exe], input=blob, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    buf = out.stdout
    mats = np.frombuffer(buf, "f4", 27 * its, 0).reshape(3, its, 3, 3)
    sh = np.frombuffer(buf, "f4", its, 108 * its); sf = np.frombuffer(buf, "f4", its, 112 * its)
    in_h = np.frombuffer(buf, "u1", its * n, 116 * its).reshape(its, n).astype(bool)
    in_f = np.frombuffer(buf, "u1", its * n, 116 * its + its * n).reshape(its, n).astype(bool)
    assert in_h.sum(1).max() > sz.TILE
    for it in range(its):
        fl, terms = ref.check32_h(mats[0, it], mats[1, it], m)
        assert (fl == in_h[it]).all() and abs(float(sh[it]) - terms.astype("f8").sum()) <= n * 2.0 ** -20 * max(float(sh[it]), 1.0)
        fl, terms = ref.check32_f(mats[2, it], m)
        assert (fl == in_f[it]).all() and abs(float(sf[it]) - terms.astype("f8").sum()) <= n * 2.0 ** -20 * max(float(sf[it]), 1.0)
