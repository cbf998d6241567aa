"""The bookkeeping of the keyed record store (csrc/record_index.h) under the KeyFrameDatabase and the covisibility index: the header
through the host compiler in a stand-alone program, under sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_index_under_sanitizers(tmp_path):
    """tests/support/record_index_check.cpp: 4000 seeded random operations per payload shape (4 + 8 and 4 + 1 bytes an element) against
    a std::map model, with -fsanitize=address,undefined, run directly."""
    exe = str(tmp_path / "record_index_check")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main() { return 0; }\n",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer runtime for the host compiler")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "support", "record_index_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-1500:] + out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines[0].startswith("kfdb ") and lines[1].startswith("covis "), lines
