"""Numpy restatements and scene helpers for ccm_scene_median_depth and ccm_map_pair_geometry (tests/test_new_points_table_cpu.py).

Test infrastructure: nothing here is imported by the library.

  median_ref       KeyFrame::ComputeSceneMedianDepth(2) on table columns as include/ccm_hot.h defines it, with numpy's sort
  f12_bound        the per-entry bound that holds ccm_map_pair_geometry to mapping.compute_f12
"""
import numpy as np

LIVE, BAD, HAS_OBS = 1, 2, 4
F4, F8 = np.float32, np.float64


def depths_ref(mp_id, pos, flags, Tcw):
    """The counted depths (float32), in feature order."""
    ids = np.asarray(mp_id, "i8"); pos = np.asarray(pos, F4).reshape(-1, 3); flags = np.asarray(flags, "u1")
    T = np.asarray(Tcw, F4).reshape(3, 4)
    ok = (ids >= 0) & (ids < len(pos))
    ids = ids[ok]
    ids = ids[(flags[ids] & LIVE) != 0]
    P = pos[ids].astype(F8)
    with np.errstate(all="ignore"):
        z = ((F8(T[2, 0]) * P[:, 0] + F8(T[2, 1]) * P[:, 1] + F8(T[2, 2]) * P[:, 2]) + F8(T[2, 3])).astype(F4)
    return z[np.isfinite(z)]


def median_ref(mp_id, pos, flags, Tcw):
    """-> (median float32, m): rank (m - 1) // 2 of the ascending depths, -0.0 before +0.0; (0, 0) when nothing counts."""
    z = depths_ref(mp_id, pos, flags, Tcw)
    if len(z) == 0:
        return F4(0), 0
    order = np.lexsort((~np.signbit(z), z))
    return z[order][(len(z) - 1) // 2], len(z)


def same_bits(a, b):
    a = np.ascontiguousarray(a, F4); b = np.ascontiguousarray(b, F4)
    return a.shape == b.shape and (a.view("u4") == b.view("u4")).all()


def f12_bound(K1, Tcw1, K2, Tcw2):
    """8 * 2^-24 * (|K1^-T| |[t12]x| |R12| |K2^-1|)_ij: two entries of K^-1 off by one float ulp (one on either side) and the three
    re-roundings of the product chain, each at most 2^-24 relative to the absolute product, with a factor 8 / 5 to spare."""
    T1, T2 = np.asarray(Tcw1, F8).reshape(3, 4), np.asarray(Tcw2, F8).reshape(3, 4)
    R12 = T1[:, :3] @ T2[:, :3].T
    t12 = -R12 @ T2[:, 3] + T1[:, 3]
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Ki = lambda K: np.array([[1 / K[0], 0, -K[2] / K[0]], [0, 1 / K[1], -K[3] / K[1]], [0, 0, 1.0]])  # noqa: E731
    K1, K2 = np.asarray(K1, F8), np.asarray(K2, F8)
    return 8.0 * 2.0 ** -24 * (np.abs(Ki(K1).T) @ np.abs(tx) @ np.abs(R12) @ np.abs(Ki(K2)))
