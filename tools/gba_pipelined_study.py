#!/usr/bin/env python3
"""CPU study (scipy) for the reduced solve of the global BA, config 5, on the reduced camera system of a late LM trial:
  1. classic PCG against the pipelined PCG of Ghysels & Vanroose (one global reduction per iteration, the preconditioner and
     the mat-vec applied to w = A u instead of r): iterations to the relative residual `--tol`, the TRUE residual
     |b - A x| / |b| reached, and the floor the recurrences reach when asked for 1e-13;
  2. the same with hat functions over 8 instead of 16 keyframes in the coarse space;
  3. the keyframe-segment-sharded solve VERDICT r2 #5 asks to price: additive Schwarz over N contiguous keyframe segments,
     each applying the exact inverse of its own diagonal block, plus the shipped coarse level: outer iterations for N = 2, 4, 8.
The system is cached in /tmp (the oracle needs ~1 min to reach the late trial).
usage: python3 tools/gba_pipelined_study.py [--iters 8] [--lam 0.042] [--tol 1e-7]"""
import argparse, os, sys, time
import numpy as np, scipy.sparse as sp, scipy.sparse.linalg as spla
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser(); ap.add_argument("--iters", type=int, default=8); ap.add_argument("--lam", type=float, default=0.042)
ap.add_argument("--tol", type=float, default=1e-7); ap.add_argument("--segments", action="store_true"); a = ap.parse_args()
cache = "/tmp/gba_late_system_%d_%g.npz" % (a.iters, a.lam)
if os.path.exists(cache):
    z = np.load(cache); Hs = sp.csr_matrix((z["data"], z["indices"], z["indptr"]), shape=tuple(z["shape"])); b = z["b"]; tt = z["tt"]
else:
    from motioncheck_ccm_slam_amd import synth
    from oracle import oracle_py as O
    g = synth.gba_graph(); t = time.time()
    if a.iters > 0:
        r = O.ba_solve(g, a.iters, 0.0)
        g = dict(g); g["poses"] = r["poses"]; g["points"] = r["points"]
        print("oracle: %d iterations, chi2 %.1f -> %.1f, %.1f s" % (r["iterations_done"], r["chi2_initial"], r["chi2_final"], time.time() - t))
    H, b, fi = O.ba_reduced_system(g, 0.0, a.lam)
    Hs = sp.csr_matrix(H); del H
    Hs = (sp.triu(Hs) + sp.triu(Hs, 1).T).tocsr()
    poses = np.asarray(g["poses"]); free = np.where(np.asarray(g["fixed"]) == 0)[0]; tt = poses[free, 4:7]
    np.savez(cache, data=Hs.data, indices=Hs.indices, indptr=Hs.indptr, shape=np.array(Hs.shape), b=b, tt=tt)
n = len(b); nf = n // 6; bb = b @ b
print("reduced system: n = %d, nnz = %d" % (n, Hs.nnz))

CL = 8
ncl = (nf + CL - 1) // CL
Minv = [np.linalg.inv(Hs[6 * c * CL:min(n, 6 * (c + 1) * CL), 6 * c * CL:min(n, 6 * (c + 1) * CL)].toarray()) for c in range(ncl)]
def cluster_apply(r):
    z = np.empty_like(r)
    for c in range(ncl):
        i0, i1 = 6 * c * CL, min(n, 6 * (c + 1) * CL); z[i0:i1] = Minv[c] @ r[i0:i1]
    return z
def hat_cols_centred(per):
    na = (nf + per - 1) // per
    cen = np.array([tt[I * per:min(nf, (I + 1) * per)].mean(0) for I in range(na)])
    rows, cols, vals = [], [], []
    for f in range(nf):
        x = (f + 0.5) / per - 0.5; I = int(np.floor(x)); al = x - I
        i0, i1, w0, w1 = min(max(I, 0), na - 1), min(I + 1, na - 1), 1 - al, al
        if i0 == i1: w0, w1 = 1.0, 0.0
        for (ag, wt) in ((i0, w0), (i1, w1)):
            if wt == 0: continue
            for d in range(6): rows.append(6 * f + d); cols.append(7 * ag + d); vals.append(wt)
            for d in range(3): rows.append(6 * f + 3 + d); cols.append(7 * ag + 6); vals.append(wt * (tt[f, d] - cen[ag, d]))
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, 7 * na))
def coarse(per):
    Rt = hat_cols_centred(per); Ac = (Rt.T @ (Hs @ Rt)).toarray(); Aci = np.linalg.inv(Ac)
    return lambda r: Rt @ (Aci @ (Rt.T @ r))
def two_level(per):
    co = coarse(per); return lambda r: cluster_apply(r) + co(r)

def pcg(prec, tol, maxit=3000):
    x = np.zeros(n); r = b.copy(); z = prec(r); p = z.copy(); rz = r @ z
    for it in range(1, maxit + 1):
        Ap = Hs @ p; al = rz / (p @ Ap); x += al * p; r -= al * Ap
        if r @ r <= tol * tol * bb: return it, x
        z = prec(r); rz2 = r @ z; p = z + (rz2 / rz) * p; rz = rz2
    return maxit, x
def ppcg(prec, tol, maxit=3000):
    """Ghysels & Vanroose, Alg. 4: gamma = (r,u), delta = (w,u) reduced together; m = M^-1 w, nn = A m need no reduction"""
    x = np.zeros(n); r = b.copy(); u = prec(r); w = Hs @ u
    zv = np.zeros(n); q = np.zeros(n); s = np.zeros(n); p = np.zeros(n)
    gam_old = al_old = 1.0
    for it in range(1, maxit + 1):
        gam = r @ u; dl = w @ u; rr = r @ r
        if rr <= tol * tol * bb: return it - 1, x
        m = prec(w); nn = Hs @ m
        if it > 1: be = gam / gam_old; al = gam / (dl - be * gam / al_old)
        else: be = 0.0; al = gam / dl
        zv = nn + be * zv; q = m + be * q; s = w + be * s; p = u + be * p
        x += al * p; r -= al * s; u -= al * q; w -= al * zv
        gam_old, al_old = gam, al
    return maxit, x
def true_res(x): return np.linalg.norm(b - Hs @ x) / np.sqrt(bb)

for per in (16, 8):
    prec = two_level(per)
    for name, fn in (("classic PCG", pcg), ("pipelined PCG", ppcg)):
        for tol in (a.tol, 1e-9, 1e-13):
            t = time.time(); it, x = fn(prec, tol, 1500)
            print("hats over %2d keyframes  %-14s tol %.0e: %4d iterations, true residual %.2e  (%.1f s)" % (per, name, tol, it, true_res(x), time.time() - t))

if a.segments:
    co = coarse(16)
    for N in (2, 4, 8):
        cuts = [6 * (nf * k // N) for k in range(N + 1)]
        lus = [spla.splu(sp.csc_matrix(Hs[cuts[k]:cuts[k + 1], cuts[k]:cuts[k + 1]])) for k in range(N)]
        def seg(r):
            z = np.empty_like(r)
            for k in range(N): z[cuts[k]:cuts[k + 1]] = lus[k].solve(r[cuts[k]:cuts[k + 1]])
            return z
        for name, prec in (("segment inverses alone", seg), ("segment inverses + coarse level", lambda r: seg(r) + co(r))):
            it, x = pcg(prec, a.tol, 1500)
            print("N = %d keyframe segments, %-32s %4d outer iterations, true residual %.2e" % (N, name, it, true_res(x)))
