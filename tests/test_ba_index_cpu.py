"""Host edge index of the bundle adjustment (csrc/ba_index.h), checked without a GPU and without the library.

tests/support/ba_index_check.cpp includes the header, builds small edge lists itself and compares every field of the result with
the slow, obvious construction: a std::stable_sort of the local edge ids by (landmark, keyframe) and counting loops.  Everything
compared is an integer or a copied double, so every comparison is exact; the harness exits 1 at the first mismatch.  Base case:
7 keyframes of which 3 are fixed, 12 landmarks of which 0, 5 and 11 have no observation, one landmark seen by fixed keyframes
only, one (landmark, keyframe) pair twice."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ba_index") / "ba_index_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "support", "ba_index_check.cpp"), "-o", exe])
    return exe


def _run(exe, mode):
    out = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", out.stdout)}


def test_sorted_input_is_used_where_it_lies_and_shuffled_input_gets_the_stable_sort(harness):
    r = _run(harness, "order")
    assert 36 <= r["edges"] <= 44
    assert r["sorted_direct"] == 1 and r["shuffled_direct"] == 0


def test_shard_keeps_only_local_edges_and_rebases_landmarks(harness):
    r = _run(harness, "shard")                                  # l0 = 4, l1 = 9
    assert r["direct"] == 0 and 0 < r["kept"] < r["edges"]
    assert r["pt_min"] == 0 and r["pt_max"] == 4                # landmarks 4 and 8 have observations


def test_all_keyframes_fixed(harness):
    r = _run(harness, "all_fixed")
    assert r["nfree"] == 0 and r["n_pose_edges"] == 0 and r["pose_first_size"] == 1 and r["pose_first0"] == 0


def test_empty_lists(harness):
    r = _run(harness, "empty")
    assert r["e0_E"] == 0 and r["e0_pt_first_size"] == 13 and r["e0_pt_first_max"] == 0
    assert r["l0_pt_first_size"] == 1 and r["l0_pt_first0"] == 0


def test_lowest_out_of_range_edge_is_reported(harness):
    r = _run(harness, "range")                                  # bad indices at edges 9 and 23
    assert r["a_1thread"] == 9 and r["a_8threads"] == 9 and r["b_1thread"] == 9 and r["b_8threads"] == 9


def test_eight_threads_give_what_one_thread_gives(harness):
    r = _run(harness, "threads")
    assert r["threads_ok"] == 1 and r["big_edges"] == 20000 and r["big_direct"] == 0
