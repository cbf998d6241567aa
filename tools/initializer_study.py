#!/usr/bin/env python3
"""Tolerance study for the monocular Initializer (CPU only): what float32 storage costs against the float64 restatement of
src/Initializer.cpp on the GPU test's own scenes, draws and seed (tests/initializer_ref.py: CASES, SEED).

The library stores its matrices in float32 like the reference and takes every null vector from an eigen-decomposition in double of
A^T A of the float matrix.  tests/initializer_ref.py emulates exactly that with numpy (LAPACK's eigh instead of Jacobi sweeps, numpy's
inverse: both differ from the library at double rounding, far below float storage) and this tool compares the emulation with the
float64 restatement:

  matrices   max |A/|A|_F -+ B/|B|_F| of H21, H12, F21 over every non-degenerate set ((s8 - s9) / s1 >= 1e-4 of the set's own
             design matrix in float64)
  flags      inlier flags that differ outside ambiguous pairs (chi-square of either direction within a relative 1e-3 of its threshold),
             and the shares of ambiguous pairs and degenerate sets of the reference alone
  CheckRT    for every motion candidate of each case's chosen model (float64 pipeline, candidates rounded to float32): flags that
             differ outside ambiguous matches, |X - X_ref|inf / depth over matches good in both, |parallax - parallax_ref| in degrees

The GPU test's bounds are 4 x the worst values printed here (tests/test_initializer_gpu.py, DESIGN.md "Initializer")."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import initializer_ref as ref  # noqa: E402


def main():
    diffs = []; pairs = amb_n = deg_n = sets_n = wrong_flags = 0
    rt_x = 0.0; rt_par = 0.0; rt_n = rt_amb = rt_wrong = 0
    for (n, share, kind, its), (p, d) in zip(ref.CASES, ref.make_cases()):
        first, second, m = ref.matches_of(p)
        sets = ref.sample_sets(len(first), d)
        ev = ref.evaluate(p, sets); em = ref.emulate(p, sets)
        ok_h = ev["gap_h"] >= 1e-4; ok_f = ev["gap_f"] >= 1e-4
        for name, ok in (("H21", ok_h), ("H12", ok_h), ("F21", ok_f)):
            diffs.append(ref.unit_aligned_diff(em[name], ev[name])[ok])
        amb_h, amb_f = ref.ambiguous_pairs(ev)
        for ok, amb, key, model in ((ok_h, amb_h, "inlier_h", 0), (ok_f, amb_f, "inlier_f", 1)):
            flags = np.zeros_like(ev[key])
            for it in range(len(sets)):
                flags[it] = ref.check32_h(em["H21"][it], em["H12"][it], m)[0] if model == 0 else ref.check32_f(em["F21"][it], m)[0]
            wrong_flags += int(((flags != ev[key]) & ~amb & ok[:, None]).sum())
            pairs += amb.size; amb_n += int(amb.sum()); deg_n += int((~ok).sum()); sets_n += len(ok)
        # CheckRT of the float64 pipeline's candidates
        SH, SF, bh, bf, model = ref.select(ev["score_h"], ev["score_f"])
        b = bh if model == 0 else bf
        if b < 0:
            continue
        mask = (ev["inlier_h"] if model == 0 else ev["inlier_f"])[b]
        cands = ref.candidates_h(ev["H21"][b], p["K"]) if model == 0 else ref.candidates_f(ev["F21"][b], p["K"])
        for R, t in cands:
            R32 = R.astype("f4"); t32 = t.astype("f4")
            r = ref.check_rt(R32, t32, p["K"], m, mask); e = ref.emulate_check_rt(R32, t32, p["K"], m, mask)
            amb = ref.ambiguous_rt(r) & mask
            rt_n += int(mask.sum()); rt_amb += int(amb.sum())
            rt_wrong += int((((e["good"] != r["good"]) | (e["triangulated"] != r["triangulated"])) & ~amb).sum())
            both = e["good"] & r["good"]
            if both.any():
                rt_x = max(rt_x, float((np.abs(e["X"][both] - r["X"][both]).max(1) / np.abs(r["X"][both, 2])).max()))
            if abs(e["n_good"] - r["n_good"]) == 0 and r["n_good"] > 0:
                rt_par = max(rt_par, abs(e["parallax"] - r["parallax"]))
    dd = np.concatenate(diffs)
    print("matrices: %d compared, median %.3g, 99th percentile %.3g, maximum %.3g" % (len(dd), np.median(dd), np.percentile(dd, 99), dd.max()))
    print("flags: %d differ outside ambiguous pairs and degenerate sets; ambiguous %d of %d pairs (%.4f %%), degenerate %d of %d sets (%.2f %%)"
          % (wrong_flags, amb_n, pairs, 100.0 * amb_n / pairs, deg_n, sets_n, 100.0 * deg_n / sets_n))
    print("CheckRT: %d flags differ outside ambiguous matches; ambiguous %d of %d; worst |dX|inf / depth %.3g, worst parallax difference %.3g deg"
          % (rt_wrong, rt_amb, rt_n, rt_x, rt_par))
    print("bounds for tests/test_initializer_gpu.py (4 x worst): matrices %.3g, X %.3g, parallax %.3g deg" % (4 * dd.max(), 4 * rt_x, 4 * rt_par))


if __name__ == "__main__":
    main()
