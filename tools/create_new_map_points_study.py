#!/usr/bin/env python3
"""Tolerance study for ccm_create_new_map_points (CPU only): what float32 storage in the operation order of csrc/map_math.h costs
against the float64 restatement of src/Mapping.cpp:363-448, on the GPU test's own scene and seed (tests/create_new_map_points_ref.py).

The pairs are the ones the GPU test sees: the oracle's SearchForTriangulation of the current keyframe, with the map-point flags as
they stand on entry, against every neighbour the baseline rule keeps (the library's match half is exact, so these are its pairs), plus
the small cases.  tests/create_new_map_points_ref.emulate_pairs32 restates map_pair with numpy (LAPACK's eigh instead of the Jacobi
sweeps: both work in double on the same A^T A, far below float storage).  Printed:

  ambiguous   share of pairs with a gate within its band (1e-5 absolute for the cosines and depth / |X - O|, 1e-3 relative for the
              reprojection tests, 1e-4 relative for the scale tests) in the float64 evaluation
  differ      statuses that differ outside the bands (must be 0)
  worst       |X - X_ref|inf / depth over the pairs that pass every gate in both

The same figures are printed for the pairs of the CPU test (tests/test_create_new_map_points_cpu.py feeds every pair of the scene
that observes one 3-D point to the host build of map_math.h, matcher or not; among them are pairs of lower parallax than the matcher
lets through, so their worst value is larger).  Each test's bound on the point is 4 x the worst value of its own pairs (DESIGN.md
"CreateNewMapPoints")."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import create_new_map_points_ref as ref  # noqa: E402
from oracle import oracle_py  # noqa: E402


def oracle_search(scene, k, has_mp1):
    cur, kf = scene["current"], scene["neighbours"][k]
    ex, ey = ref.epipole32(cur, kf)
    z1 = np.zeros(len(cur["kp_x"]), "f4"); z2 = np.zeros(len(kf["kp_x"]), "f4")
    return oracle_py.search_for_triangulation(cur["desc"], cur["node"], has_mp1, cur["kp_x"], cur["kp_y"], z1, kf["desc"], kf["node"],
                                              kf["has_mp"], kf["kp_x"], kf["kp_y"], z2, kf["kp_octave"], scene["F12"][k], ex, ey,
                                              kf["scale_factors"], kf["level_sigma2"], 0)[1]


def study(label, jobs):
    """jobs: (kf1, kf2, i1, i2) per neighbour -> (differ, worst)"""
    pairs = amb_n = differ = 0
    worst = 0.0
    counts = np.zeros(len(ref.STATUS), "i8")
    for k, (cur, kf, i1, i2) in enumerate(jobs):
        r = ref.pairs_ref(cur, kf, i1, i2); e = ref.emulate_pairs32(cur, kf, i1, i2)
        pairs += len(i1); amb_n += int(r["ambiguous"].sum())
        bad = (r["status"] != e["status"]) & ~r["ambiguous"]
        differ += int(bad.sum())
        for j in np.flatnonzero(bad)[:5]:
            print("  differs: job %d pair (%d, %d): float64 %s, float32 %s" % (k, i1[j], i2[j], ref.STATUS[r["status"][j]], ref.STATUS[e["status"][j]]))
        both = (r["status"] == ref.S["OK"]) & (e["status"] == ref.S["OK"])
        if both.any():
            worst = max(worst, float((np.abs(e["X"][both].astype("f8") - r["X"][both]).max(1) / np.abs(r["z1"][both])).max()))
        counts += np.bincount(r["status"], minlength=len(ref.STATUS))
    print("%s: %d pairs: " % (label, pairs) + ", ".join("%s %d" % (ref.STATUS[s], counts[s]) for s in np.flatnonzero(counts)))
    print("  ambiguous %d of %d pairs (%.3f %%)" % (amb_n, pairs, 100.0 * amb_n / max(pairs, 1)))
    print("  statuses that differ outside the bands: %d" % differ)
    print("  worst |dX|inf / depth over pairs OK in both: %.3g  ->  bound (4 x): %.3g" % (worst, 4 * worst))
    return differ


def main():
    oracle_py.lib()
    scene = ref.make_scene()
    matched, true = [], []
    for sc in [scene] + [ref.make_small(scene, n1, ks, **kw) for n1, ks, kw in ref.SMALL_CASES]:
        cur = sc["current"]
        for k, kf in enumerate(sc["neighbours"]):
            if ref.baseline_too_short(cur["Ow"], kf["Ow"], sc["median_depth"][k]) or len(kf["kp_x"]) == 0:
                continue
            m12 = oracle_search(sc, k, cur["has_mp"])
            i1 = np.flatnonzero(m12 >= 0)
            matched.append((cur, kf, i1, m12[i1]))
            if sc is scene:
                true.append((cur, kf) + ref.true_pairs(scene, k))
    differ = study("GPU test (the matcher's pairs of the scene and the small cases)", matched)
    differ += study("CPU test (every pair of the scene that observes one point, neighbours the baseline rule keeps)", true)
    return 0 if differ == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
