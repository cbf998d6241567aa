"""The per-neighbour inputs of CreateNewMapPoints, defined on the host: ccm_scene_median_depth and ccm_map_pair_geometry against
numpy restatements, csrc/map_math.h in a stand-alone program under the address and undefined-behaviour sanitizers
(tests/support/map_geometry_check.cpp, which also selects the rank bit by bit over the depth keys, the way a workgroup would), and
the stability of the header and the binding.

F12 is held two ways: to the float64 ref.f12_64 through the distance of noise-free projections from their epipolar lines (< 0.01 px,
the tolerance test_create_new_map_points_cpu.py uses for mapping.compute_f12), and to mapping.compute_f12 entry by entry within
nref.f12_bound.  The epipole is bit-equal to mapping.compute_epipole."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib, mapping
import create_new_map_points_ref as ref
import new_points_table_ref as nref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F4 = np.float32
LIVE, BAD, HAS_OBS = nref.LIVE, nref.BAD, nref.HAS_OBS


@pytest.fixture(scope="module")
def scene():
    return ref.make_scene()


def _pose(rng, tz=0.0):
    T = ref._pose(ref.rodrigues(rng.normal(0, 0.05, 3)), rng.normal(0, 0.3, 3)).astype(F4)
    T[2, 3] += F4(tz)
    return T


def median_cases():
    """-> [(name, mp_id, pos, flags, Tcw)]: m = 0, 1, 2, 3, 4, 63, 64, 65 among features that do not count (ids of -1 and beyond the
    capacity, rows that are not LIVE), BAD rows that do count, all depths equal, ties straddling the median rank, negative depths,
    zeros of both signs, a NaN position and an infinite one."""
    rng = np.random.default_rng(11)
    cap = 300
    pos = np.stack([rng.uniform(-6, 6, cap), rng.uniform(-3, 3, cap), rng.uniform(4, 14, cap)], 1).astype(F4)
    flags = np.full(cap, LIVE | HAS_OBS, np.uint8)
    flags[200:220] = 0                                      # not LIVE
    flags[220:240] = HAS_OBS | BAD                          # not LIVE either
    flags[100:130] = LIVE | BAD                             # BAD rows count
    cases = []
    for m in (0, 1, 2, 3, 4, 63, 64, 65):
        live = rng.choice(np.r_[0:200, 240:cap], m, replace=False)
        ids = np.concatenate([live, [-1, cap, cap + 7, -5, 205, 230]]).astype("i4")
        cases.append(("m=%d" % m, ids[rng.permutation(len(ids))], pos, flags, _pose(rng)))
    cases.append(("bad rows count", np.arange(90, 140).astype("i4"), pos, flags, _pose(rng)))
    cases.append(("one slot held by every feature", np.full(17, 42, "i4"), pos, flags, _pose(rng)))
    I = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(F4)
    tie = pos.copy(); tie[:10, 2] = [1, 2, 3, 5, 5, 5, 5, 7, 8, 9]
    cases.append(("ties straddle the rank", np.arange(10).astype("i4"), tie, flags, I))
    cases.append(("ties below the rank", np.array([3, 4, 0, 1, 2, 7], "i4"), tie, flags, I))
    cases.append(("negative depths", rng.integers(0, 200, 41).astype("i4"), pos, flags, _pose(rng, tz=-9.0)))
    cases.append(("every depth negative", rng.integers(0, 200, 40).astype("i4"), pos, flags, _pose(rng, tz=-100.0)))
    z = pos.copy(); z[:6, 2] = [0.0, -0.0, 0.0, -0.0, -0.0, 1.0]; z[:6, :2] = -1.0     # 0 * -1 = -0: the sum keeps the sign of z
    Iz = I.copy(); Iz[2, 3] = -0.0
    cases.append(("zeros of both signs", np.arange(5).astype("i4"), z, flags, Iz))
    cases.append(("zeros, even count", np.arange(4).astype("i4"), z, flags, Iz))
    bad = pos.copy(); bad[3] = np.nan; bad[5, 2] = np.inf; bad[6, 0] = -np.inf
    cases.append(("non-finite positions", np.arange(12).astype("i4"), bad, flags, _pose(rng)))
    cases.append(("only a NaN", np.array([3], "i4"), bad, flags, _pose(rng)))
    cases.append(("no feature", np.zeros(0, "i4"), pos, flags, _pose(rng)))
    return cases


def pair_cases(scene):
    """-> [(K1, Tcw1, Ow1, K2, Tcw2)]: the scene's 21 pairs, and pairs with two different cameras whose principal points and focal
    lengths have full float mantissas"""
    cur = scene["current"]
    out = [(cur["K"], cur["Tcw"], cur["Ow"], kf["K"], kf["Tcw"]) for kf in scene["neighbours"]]
    rng = np.random.default_rng(3)
    for _ in range(40):
        K1 = np.array([rng.uniform(300, 900), rng.uniform(300, 900), rng.uniform(200, 500), rng.uniform(150, 350)], F4)
        K2 = np.array([rng.uniform(300, 900), rng.uniform(300, 900), rng.uniform(200, 500), rng.uniform(150, 350)], F4)
        kf = scene["neighbours"][int(rng.integers(1, 21))]
        out.append((K1, cur["Tcw"], cur["Ow"], K2, kf["Tcw"]))
    return out


def _mkf(K, Tcw, Ow=None):
    T = np.asarray(Tcw, F4).reshape(3, 4)
    Ow = (-T[:, :3].astype("f8").T @ T[:, 3].astype("f8")).astype(F4) if Ow is None else Ow
    z = np.zeros(0)
    return mapping.MapKeyFrame(z, z, z, np.zeros((0, 32)), z, z, K, T, Ow, ref.SCALE_FACTORS, ref.LEVEL_SIGMA2)


def _build(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", *extra,
                           os.path.join(ROOT, "tests", "support", "map_geometry_check.cpp"), "-o", exe])
    return exe


def test_median_depth_equals_the_numpy_restatement():
    seen_m = set()
    for name, ids, pos, flags, T in median_cases():
        got, m = mapping.scene_median_depth(ids, pos, flags, T)
        want, wm = nref.median_ref(ids, pos, flags, T)
        assert m == wm and nref.same_bits(got, want), (name, got, m, want, wm)
        seen_m.add(m)
    assert {0, 1, 2, 3, 4, 63, 64, 65} <= seen_m
    by = {c[0]: c for c in median_cases()}
    assert mapping.scene_median_depth(*by["ties straddle the rank"][1:])[0] == 5.0           # rank 4 of 1 2 3 5 5 5 5 7 8 9
    assert mapping.scene_median_depth(*by["ties below the rank"][1:])[0] == 3.0              # rank 2 of 1 2 3 5 5 7
    z = mapping.scene_median_depth(*by["zeros of both signs"][1:])[0]                        # -0 -0 -0 +0 +0: rank 2
    assert z == 0 and np.signbit(z)
    z = mapping.scene_median_depth(*by["zeros, even count"][1:])[0]                          # -0 -0 +0 +0: rank 1
    assert z == 0 and np.signbit(z)
    assert mapping.scene_median_depth(*by["every depth negative"][1:])[0] < 0
    assert mapping.scene_median_depth(*by["non-finite positions"][1:])[1] == 9
    assert mapping.scene_median_depth(*by["only a NaN"][1:]) == (0.0, 0)
    assert mapping.scene_median_depth(*by["bad rows count"][1:])[1] == 50


def test_pair_geometry_against_float64_and_the_python_helpers(scene):
    cur = scene["current"]
    worst = 0.0
    for j, (K1, T1, O1, K2, T2) in enumerate(pair_cases(scene)):
        F, e = mapping.pair_geometry(K1, T1, O1, K2, T2)
        assert F.shape == (3, 3) and F.dtype == F4 and e.dtype == F4
        k1, k2 = _mkf(K1, T1, O1), _mkf(K2, T2)
        Fpy = mapping.compute_f12(k1, k2)
        bound = nref.f12_bound(K1, T1, K2, T2)
        diff = np.abs(F.astype("f8") - Fpy.astype("f8"))
        worst = max(worst, float((diff / bound).max()))
        assert (diff <= bound).all(), (j, diff / bound)
        assert nref.same_bits(e, mapping.compute_epipole(k1, k2)), j
        if j < len(scene["neighbours"]):
            assert nref.same_bits(e, ref.epipole32(cur, scene["neighbours"][j]))
        # noise-free projections lie on their epipolar lines: within 0.01 px, as for compute_f12
        P = scene["X"][:200]
        proj = lambda K, T: (K[0] * (P @ T[0, :3] + T[0, 3]) / (P @ T[2, :3] + T[2, 3]) + K[2], K[1] * (P @ T[1, :3] + T[1, 3]) / (P @ T[2, :3] + T[2, 3]) + K[3])  # noqa: E731
        u1, v1 = proj(np.asarray(K1, "f8"), np.asarray(T1, "f8").reshape(3, 4)); u2, v2 = proj(np.asarray(K2, "f8"), np.asarray(T2, "f8").reshape(3, 4))
        line = np.stack([u1, v1, np.ones(len(P))], 1) @ F.astype("f8")
        dist = np.abs(line[:, 0] * u2 + line[:, 1] * v2 + line[:, 2]) / np.hypot(line[:, 0], line[:, 1])
        assert dist.max() < 0.01, (j, float(dist.max()))
    print("worst |F12 - compute_f12| / bound: %.3g" % worst)


def test_host_program_under_the_sanitizers(tmp_path, scene):
    """The same records through tests/support/map_geometry_check.cpp: bit-equal to the library's exports, the bit-by-bit rank
    selection over the keys agrees with the sort, and the program built with -fsanitize=address,undefined runs clean."""
    med, pairs = median_cases(), pair_cases(scene)
    blob = b""
    for K1, T1, O1, K2, T2 in pairs:
        blob += np.int32(0).tobytes() + b"".join(np.ascontiguousarray(a, F4).tobytes() for a in (K1, T1, O1, K2, T2))
    for name, ids, pos, flags, T in med:
        blob += np.array([1, len(ids), len(pos)], "i4").tobytes() + ids.tobytes() + np.ascontiguousarray(pos, F4).tobytes() + flags.tobytes() + T.tobytes()
    out = subprocess.run([_build(tmp_path, "map_geometry_check")], input=blob, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    buf, off = out.stdout, 0
    for K1, T1, O1, K2, T2 in pairs:
        F = np.frombuffer(buf, F4, 9, off); e = np.frombuffer(buf, F4, 2, off + 36); off += 44
        wF, we = mapping.pair_geometry(K1, T1, O1, K2, T2)
        assert nref.same_bits(F, wF.reshape(9)) and nref.same_bits(e, we)
    for name, ids, pos, flags, T in med:
        m1 = np.frombuffer(buf, F4, 1, off)[0]; n1 = int(np.frombuffer(buf, "i4", 1, off + 4)[0])
        m2 = np.frombuffer(buf, F4, 1, off + 8)[0]; n2 = int(np.frombuffer(buf, "i4", 1, off + 12)[0]); off += 16
        want, wm = nref.median_ref(ids, pos, flags, T)
        assert n1 == n2 == wm and nref.same_bits(m1, want) and nref.same_bits(m2, want), name
    assert off == len(buf)
    san = subprocess.run([_build(tmp_path, "map_geometry_check_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))],
                         input=blob, capture_output=True, timeout=300)
    assert san.returncode == 0 and san.stderr == b"", san.stderr[-2000:]
    assert san.stdout == out.stdout


def test_null_arguments_are_refused():
    lib = _lib.load()
    a = np.zeros(12, F4); i = np.zeros(4, "i4"); q = _lib.ptr
    assert lib.ccm_map_pair_geometry(q(a), q(a), q(a), q(a), q(a), q(a), None) == -1
    assert lib.ccm_map_pair_geometry(None, q(a), q(a), q(a), q(a), q(a), q(a)) == -1
    assert lib.ccm_scene_median_depth(-1, q(i), 1, q(a), q(a.view("u1")), q(a), q(a), q(i)) == -1
    assert lib.ccm_scene_median_depth(1, None, 1, q(a), q(a.view("u1")), q(a), q(a), q(i)) == -1
    assert lib.ccm_scene_median_depth(1, q(i), 1, q(a), q(a.view("u1")), q(a), None, q(i)) == -1
    med = np.full(1, 7, F4); m = np.full(1, 7, "i4")                              # a table without rows: nothing counts
    assert lib.ccm_scene_median_depth(4, q(i), 0, None, None, q(a), q(med), q(m)) == 0 and med[0] == 0 and m[0] == 0


def test_abi_is_stable(tmp_path):
    """The new symbols exist, the ABI version stays 3, and the structures the header had keep their sizes and agree with the binding
    (a C program prints what the header gives)."""
    lib = _lib.load()
    new = ("ccm_map_pair_geometry", "ccm_scene_median_depth")
    for name in new:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.ccm_abi_version() == 3 == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "ccm_hot.h")).read()
    assert re.search(r"#define CCM_ABI_VERSION 3\b", header)
    for name in new:
        assert len(re.findall(r"^int\s+%s\s*\(" % name, header, re.M)) == 1, name
    names = ["ccm_map_keyframe", "ccm_new_points_problem", "ccm_new_points_tap", "ccm_new_points_result", "ccm_new_points_frames",
             "ccm_map_update", "ccm_map_refresh", "ccm_map_refresh_result"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ccm_hot.h"\nint main(void) {\n'
                   + "".join('  printf("%%zu\\n", sizeof(%s));\n' % n for n in names)
                   + '  return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).split("\n")
    sizes = [int(x) for x in lines[:len(names)]]
    binding = [_lib.MapKeyframe, _lib.NewPointsProblem, _lib.NewPointsTap, _lib.NewPointsResult, _lib.NewPointsFrames, _lib.MapUpdate,
               _lib.MapRefresh, _lib.MapRefreshResult]
    assert sizes == [C.sizeof(s) for s in binding]
    assert sizes == [112, 48, 24, 56, 48, 64, 96, 32]                           # what they were before these exports were added
