"""Hat functions of the PCG's coarse space (csrc/ba_pcg.h), checked without a GPU and without the library.

tests/support/ba_pcg_check.cpp includes the header and walks nfree = 1 .. 699 and 1999, 2000, 2048, 4095, 4096, 5000, 8191, 8192,
8193, 10000, 16384 free keyframes with A = PCG_CL * pcg_agg_clusters(nfree) keyframes per aggregate and nagg = ceil(nfree / A):
pcg_hat's weights add up to exactly 1 (multiples of 1 / (2A), A a power of two) and its aggregates satisfy 0 <= i0 <= i1 < nagg;
pcg_hat_weight(f, I) is non-zero exactly for the keyframes of pcg_hat_support(I); the coarse dimension PCG_CDOF * nagg stays within
PCG_COARSE_MAX; pcg_agg_clusters gives 2, 4 or 8.  k_pcg_coarse_build, k_ppcg_prec and ppcg_contribute rest on these.  The harness
exits 1 at the first mismatch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = list(range(1, 700)) + [1999, 2000, 2048, 4095, 4096, 5000, 8191, 8192, 8193, 10000, 16384]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ba_pcg") / "ba_pcg_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "support", "ba_pcg_check.cpp"), "-o", exe])
    return exe


def test_hat_functions_partition_unity_and_match_their_supports(harness):
    out = subprocess.run([harness], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    r = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", out.stdout)}
    assert r["sizes"] == len(SIZES) and r["keyframes"] == sum(SIZES)            # every size and every keyframe was visited
    # 7 * ceil(nfree / (8 agg)) <= 1792 holds up to nfree = 4096 with agg = 2 and up to 8192 with agg = 4
    assert (r["agg2"], r["agg4"], r["agg8"]) == (sum(n <= 4096 for n in SIZES), sum(4096 < n <= 8192 for n in SIZES), sum(n > 8192 for n in SIZES))
