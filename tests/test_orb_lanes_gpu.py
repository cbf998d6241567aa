"""The extractor's two-lane device path (orb_extract_lanes in csrc/orb_host.cpp): chunks of frames alternating between the context's
stream and its auxiliary stream must give the bytes of the unsplit call, stay ordered with what the caller queues around them, carry
the status word across lanes and calls, and step aside while profiling is on.  CCM_ORB_LANE_FRAMES is read once per process, so
every case runs in a child process of its own (as test_orb_gpu.py::test_alternative_kernel_paths does)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what every child starts with: torch first (its HIP runtime is the one the library then binds to, see conftest.py), device
# buffers as torch tensors as in bench.py, and digests of the three result arrays
PRELUDE = r'''
import ctypes as C, hashlib, json, sys
import numpy as np
import torch
torch.cuda.init()
from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.orb import ORBextractor
from oracle import oracle_py as O
lib = _lib.load()
ctx = _lib.Context(0)

def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda(); torch.cuda.synchronize(); return t

def extract(ex, t):
    b, h, w = t.shape
    ex.extract_dev(t.data_ptr(), w, h, w, w * h, b)

def digests(kps, desc, counts, n):
    return [hashlib.sha256(np.ascontiguousarray(a[:n]).tobytes()).hexdigest() for a in (counts, kps, desc)]

def same_as_oracle(par, img, kps, desc, n):
    r = O.orb_extract(par, img)
    assert n == len(r["kps"]) and (desc[:n] == r["desc"]).all()
    for name in r["kps"].dtype.names:
        assert (kps[:n][name] == r["kps"][name]).all(), name
    assert not desc[n:].any() and not kps[n:]["size"].any()          # pad rows are zero

def match_buffers(ex, n_pairs):
    out = [torch.full((n_pairs, ex.max_per_image), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    return out

def match(ex, out):
    """consecutive frame pairs of the resident descriptors, as bench.py queues them; enqueues only"""
    d, c, m = ex.result_dev()
    ctx.check(lib.ccm_hamming_match_dev(ctx.handle, C.c_void_p(d), m, C.c_size_t(m), C.c_void_p(d + m * 32), m, C.c_size_t(m), len(out[0]),
                                        C.c_void_p(c), C.c_void_p(c + 4), *[C.c_void_p(t.data_ptr()) for t in out]))
'''

SAME_BYTES = PRELUDE + r'''
ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
imgs = synth.frames(20, 7)
extract(ex, dev(imgs))
kps, desc, counts = ex.fetch()
for f in (0, 3, 6):
    same_as_oracle(O.default_params(), imgs[f], kps[f], desc[f], counts[f])
print(json.dumps(digests(kps, desc, counts, 7)))
'''

SMALL_GEOMETRY = PRELUDE + r'''
w, h, nf, sf, nl, ini, mn = 200, 160, 300, 1.2, 4, 20, 7             # test_parameter_sweep's smallest image, with fewer levels
ex = ORBextractor(nf, sf, nl, ini, mn, ctx=ctx)
imgs = np.stack([synth.frame(s, w, h) for s in range(5)])
extract(ex, dev(imgs))
kps, desc, counts = ex.fetch()
for f in range(5):
    same_as_oracle(O.default_params(nf, sf, nl, ini, mn), imgs[f], kps[f], desc[f], counts[f])
print(json.dumps("ok"))
'''

BACK_TO_BACK = PRELUDE + r'''
ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
X, Y = dev(synth.frames(20, 6)), dev(synth.frames(40, 6))
extract(ex, Y); match(ex, match_buffers(ex, 5)); ctx.sync()          # buffers, tables and the lane's events exist: the runs below only enqueue
def four_calls(fence):
    A, B = match_buffers(ex, 5), match_buffers(ex, 5)
    extract(ex, X); fence()
    match(ex, A); fence()
    extract(ex, Y); fence()
    match(ex, B); fence()
    ctx.sync()
    return [t.cpu().numpy() for t in A + B]
free = four_calls(lambda: None)                                       # no host synchronisation between the four calls
held = four_calls(ctx.sync)
assert all((a == b).all() for a, b in zip(free, held))
assert not any((a == -7).all() for a in held)                         # the matcher did write
assert any((a != b).any() for a, b in zip(held[:3], held[3:]))        # X and Y are different problems
print(json.dumps("ok"))
'''

STATUS = PRELUDE + r'''
imgs = synth.frames(20, 4)
t = dev(imgs)
small = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx, max_per_image=500)  # a frame of synth.frames yields over 900
extract(small, t)
try:
    small.fetch()
    raise SystemExit("fetch did not fail")
except _lib.CcmError as e:
    assert e.code == -4, e                                              # CCM_E_CAPACITY
ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
extract(ex, t)
kps, desc, counts = ex.fetch()                                          # the status word does not go stale
same_as_oracle(O.default_params(), imgs[3], kps[3], desc[3], counts[3]) # a frame of lane 1's chunk
print(json.dumps("ok"))
'''

PROFILING = PRELUDE + r'''
ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
imgs = synth.frames(20, 8)
t = dev(imgs)
ctx.profile(True)
extract(ex, t)
prof = ctx.profile_read()
ctx.profile(False)
launches = {k: n for k, (ms, n) in prof.items() if n}
assert launches == {"k_pyr_resize": 7, "k_fast_score": 1, "k_octree": 1, "k_orient_desc": 1}, launches    # one unsplit call
kps, desc, counts = ex.fetch()
print(json.dumps(digests(kps, desc, counts, 7)))
'''


def _child(code, lane_frames):
    env = dict(os.environ, PYTHONPATH=ROOT, CCM_ORB_LANE_FRAMES=str(lane_frames))
    return subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _result(proc):
    out, err = proc.communicate(timeout=600)
    assert proc.returncode == 0, out[-2000:] + err[-2000:]
    return json.loads(out.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def seven_frames():
    """{frames per chunk: digests of counts, keypoints and descriptors} of synth.frames(20, 7) under five schedules: 0 is the single
    lane; 1, 2 and 3 give seven, three and two chunks (odd remainders, a last chunk alone on a lane, either lane ending last); 7 is
    one chunk again.  Each child has checked frames 0, 3 and 6 against the oracle.  The five children run side by side."""
    procs = {lf: _child(SAME_BYTES, lf) for lf in (0, 1, 2, 3, 7)}
    return {lf: _result(p) for lf, p in procs.items()}


@pytest.mark.parametrize("lane_frames", [1, 2, 3, 7])
def test_same_bytes_under_every_schedule(seven_frames, lane_frames):
    assert seven_frames[lane_frames] == seven_frames[0]


def test_small_geometry_in_chunks_of_two():
    assert _result(_child(SMALL_GEOMETRY, 2)) == "ok"


def test_calls_back_to_back_with_a_consumer_in_between():
    """extract, match, extract, match without a host synchronisation: lane 1 of the second extract must not overwrite the descriptors
    the first match still reads.  A race does not fail every time: this shows the wiring, the event order in the code rules the race out."""
    assert _result(_child(BACK_TO_BACK, 2)) == "ok"


def test_status_survives_the_lanes_and_does_not_go_stale():
    assert _result(_child(STATUS, 2)) == "ok"


def test_profiling_selects_the_single_lane(seven_frames):
    assert _result(_child(PROFILING, 2)) == seven_frames[0]
