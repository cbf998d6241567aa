#!/usr/bin/env python3
"""CPU study behind the tolerances of tests/test_sim3_solver_gpu.py: Sim3Solver's hypothesis (Horn's closed form + the two
reprojection checks, src/Sim3Solver.cpp:210-348) evaluated in float32 and in float64 with numpy on inputs of the tests' shape.

  flags      how often do float32 and float64 disagree on an inlier flag, how many (hypothesis, correspondence) pairs are
             ambiguous (err / maxErr within a relative margin of 1) and how many hypotheses degenerate (top two eigenvalues of N
             within a relative gap)?  Measured: 209,400 pairs, 0 disagreements, 0.0043 % ambiguous at 1e-3, 0.3 % of 2,400
             hypotheses with a gap below 1e-3.
  estimates  float32 against float64 R, t, s over non-degenerate hypotheses.  Measured over 1,200 hypotheses: <= 1.8e-5 (R),
             <= 6.1e-5 (t, relative to max(1, |t|inf)), <= 2.8e-7 (s, relative).

No GPU and no library: numpy only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sim3_problems import rand_sim3, sim3_map  # noqa: E402


def horn(P1, P2, fix, dt, stored_scale=False):
    """P1, P2 [H][3][3], rows = points -> R [H][3][3], t [H][3], s [H], eigenvalue gap [H], all in precision dt.
    stored_scale: the two sums of the scale as src/Sim3Solver.cpp:278-292 stores them -- nom a double sum of exact products of the dt
    entries (cv::Mat::dot), den a double sum of squares rounded to dt first (cv::pow into a float matrix), the quotient rounded to dt.
    Without it both sums round alike and cancel exactly wherever Pr1 = P3, which hides the one rounding an exact input leaves."""
    P1 = P1.astype(dt); P2 = P2.astype(dt)
    O1 = P1.sum(1) / dt(3); O2 = P2.sum(1) / dt(3)
    Pr1 = P1 - O1[:, None]; Pr2 = P2 - O2[:, None]
    M = np.einsum("hki,hkj->hij", Pr2, Pr1).astype(dt)
    N = np.zeros((len(P1), 4, 4), dt)
    N[:, 0, 0] = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]; N[:, 0, 1] = M[:, 1, 2] - M[:, 2, 1]; N[:, 0, 2] = M[:, 2, 0] - M[:, 0, 2]
    N[:, 0, 3] = M[:, 0, 1] - M[:, 1, 0]; N[:, 1, 1] = M[:, 0, 0] - M[:, 1, 1] - M[:, 2, 2]; N[:, 1, 2] = M[:, 0, 1] + M[:, 1, 0]
    N[:, 1, 3] = M[:, 2, 0] + M[:, 0, 2]; N[:, 2, 2] = -M[:, 0, 0] + M[:, 1, 1] - M[:, 2, 2]; N[:, 2, 3] = M[:, 1, 2] + M[:, 2, 1]
    N[:, 3, 3] = -M[:, 0, 0] - M[:, 1, 1] + M[:, 2, 2]
    for i in range(4):
        for j in range(i):
            N[:, i, j] = N[:, j, i]
    w, v = np.linalg.eigh(N)
    q = v[:, :, 3]; gap = (w[:, 3] - w[:, 2]) / np.maximum(np.abs(w[:, 3]), dt(1e-30))
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)], -1),
                  np.stack([2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)], -1),
                  np.stack([2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)], -1)], 1).astype(dt)
    P3 = np.einsum("hij,hkj->hki", R, Pr2)
    s = np.ones(len(P1), dt) if fix else ((Pr1 * P3).sum((1, 2)) / (P3 * P3).sum((1, 2))).astype(dt)
    if stored_scale and not fix:
        P3 = P3.astype(dt)
        s = ((Pr1.astype("f8") * P3.astype("f8")).sum((1, 2)) / (P3 * P3).astype(dt).astype("f8").sum((1, 2))).astype(dt)
    t = O1 - s[:, None] * np.einsum("hij,hj->hi", R, O2)
    return R, t.astype(dt), s, gap


def proj(K, P):
    iz = 1 / P[..., 2]
    return np.stack([K[0] * (P[..., 0] * iz) + K[2], K[1] * (P[..., 1] * iz) + K[3]], -1)


def check(R, t, s, X1, X2, K1, K2, m1, m2, dt):
    X1 = X1.astype(dt); X2 = X2.astype(dt); K1 = K1.astype(dt); K2 = K2.astype(dt)
    p1 = proj(K1, X1); p2 = proj(K2, X2)
    A = s[:, None, None] * R
    q21 = np.einsum("hij,nj->hni", A, X2) + t[:, None]
    Ai = (1 / s)[:, None, None] * R.transpose(0, 2, 1); ti = -np.einsum("hij,hj->hi", Ai, t)
    q12 = np.einsum("hij,nj->hni", Ai, X1) + ti[:, None]
    d1 = p1[None] - proj(K1, q21); d2 = proj(K2, q12) - p2[None]
    e1 = (d1 * d1).sum(-1).astype(dt); e2 = (d2 * d2).sum(-1).astype(dt)
    return e1, e2, (e1 < m1[None].astype(dt)) & (e2 < m2[None].astype(dt))


K1 = np.array([458.654, 457.296, 367.215, 248.375]); K2 = np.array([435.2, 435.2, 367.4, 252.2])


def cloud(rng, n):
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2.5, 9, n)], 1)


def bounds(rng, n):
    return (np.float32(9.210) * (np.float32(1.2) ** (2 * rng.integers(0, 8, n))).astype("f4")).astype("f4")


def study_flags(H=300):
    rng = np.random.default_rng(11)
    tot = mis = nh = 0
    margins = (1e-2, 3e-3, 1e-3, 3e-4, 1e-4)
    uncovered = {m: 0 for m in margins}; amb = {m: 0 for m in margins}; gaps = {g: 0 for g in (1e-2, 1e-3, 1e-4)}
    for n, share, fix in [(20, 0.3, 0), (35, 0.5, 0), (60, 0.3, 1), (100, 0.4, 0), (150, 0.6, 0), (300, 0.5, 0), (8, 0.0, 0), (25, 0.7, 0)]:
        S = rand_sim3(rng, rot=0.5, trans=1.0, scale=0.3)
        if fix:
            S[7] = 1
        X2 = cloud(rng, n)
        X1 = sim3_map(S, X2) + rng.normal(0, 0.004, (n, 3)) * X2[:, 2:3]
        bad = rng.random(n) < share
        X1[bad] = cloud(rng, int(bad.sum()))
        X1 = X1.astype("f4"); X2 = X2.astype("f4")
        m1 = bounds(rng, n); m2 = bounds(rng, n)
        tri = np.stack([rng.permutation(n)[:3] for _ in range(H)])
        out = {}
        for dt in (np.float64, np.float32):
            R, t, s, gap = horn(X1[tri], X2[tri], fix, dt)
            out[dt] = check(R, t, s, X1, X2, K1, K2, m1, m2, dt) + (gap,)
        e1, e2, f64, gap = out[np.float64]; f32 = out[np.float32][2]
        d = f64 != f32
        tot += d.size; mis += int(d.sum()); nh += H
        r = np.minimum(np.abs(e1 / m1[None] - 1), np.abs(e2 / m2[None] - 1))
        for m in margins:
            uncovered[m] += int((d & (r >= m)).sum()); amb[m] += int((r < m).sum())
        for g in gaps:
            gaps[g] += int((gap < g).sum())
    print("flags: pairs", tot, "float32 != float64", mis)
    print("       disagreements outside the margin", uncovered)
    print("       ambiguous share by margin", {m: v / tot for m, v in amb.items()})
    print("       hypotheses with an eigenvalue gap below", gaps, "of", nh)


def study_estimates(H=300):
    rng = np.random.default_rng(12)
    rows = []
    for n, fix in [(20, 0), (60, 1), (150, 0), (300, 0)]:
        S = rand_sim3(rng, rot=0.5, trans=1.0, scale=0.3)
        X2 = cloud(rng, n)
        X1 = sim3_map(S, X2) + rng.normal(0, 0.004, (n, 3)) * X2[:, 2:3]
        bad = rng.random(n) < 0.4
        X1[bad] = X2[rng.permutation(n)][bad]
        X1 = X1.astype("f4"); X2 = X2.astype("f4")
        tri = np.stack([rng.permutation(n)[:3] for _ in range(H)])
        R, t, s, g = horn(X1[tri], X2[tri], fix, np.float64); r, tt, ss, _ = horn(X1[tri], X2[tri], fix, np.float32)
        ok = g >= 1e-3
        dR = np.abs(R - r).max((1, 2))[ok]; dt = (np.abs(t - tt).max(1) / np.maximum(1, np.abs(t).max(1)))[ok]; ds = (np.abs(s - ss) / np.abs(s))[ok]
        rows.append((n, float(dR.max()), float(dt.max()), float(ds.max())))
    print("estimates: (N, max |dR|, max |dt| / max(1, |t|), max |ds| / s)", rows)


def study_special():
    """The special inputs of tests/sim3_solver_cases.py (X1 = X2 with free and with fixed scale, X1 = diag(-1, -1, 1) X2 + t0): float32
    against float64 R, t, s over the non-collinear samples of each solver's draws.  Returns {name: (max |dR|, max |dt| / max(1, |t|),
    max |ds| / s)}; tests/test_sim3_solver_cases_gpu.py takes 4 x these as its bounds.  The float32 side forms the scale as the reference
    stores it (horn's stored_scale): at X1 = X2 that is the only rounding left, and 0 would be the bound without it."""
    import sim3_solver_cases as cases
    import sim3_solver_ref as ref
    out = {}
    for name, (p, draws) in (("identity, free scale", cases.identity(False)), ("identity, fixed scale", cases.identity(True)),
                             ("half turn", cases.half_turn())):
        n = len(p["X1"])
        tri = np.array([ref.sample_indices(n, d) for d in draws[0]])
        tri = tri[cases.non_collinear(p, tri)]
        R, t, s, g = horn(p["X1"][tri], p["X2"][tri], p["fix_scale"], np.float64)
        r, tt, ss, _ = horn(p["X1"][tri], p["X2"][tri], p["fix_scale"], np.float32, stored_scale=True)
        dR = np.abs(R - r).max((1, 2)); dt = np.abs(t - tt).max(1) / np.maximum(1, np.abs(t).max(1)); ds = np.abs(s - ss) / np.abs(s)
        out[name] = (float(dR.max()), float(dt.max()), float(ds.max()))
        print("special: %-22s %d samples, smallest eigenvalue gap %.3g, max |dR| %.3g, max |dt| / max(1, |t|) %.3g, max |ds| / s %.3g"
              % (name, len(tri), float(g.min()), *out[name]))
    return out


if __name__ == "__main__":
    with np.errstate(all="ignore"):
        study_flags()
        study_estimates()
        study_special()
