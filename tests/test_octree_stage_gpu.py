"""k_octree held to its own input: the candidates the kernel gathered (debug tap), the oracle's orc_distribute_octree on them, the
selected keys in order against the keypoints of every octave (octree_stage_ref.check_stage).  The cases walk the kernel's paths: the
one-trip gather and the loop gather (more cells than the one-trip form takes; more than OCT_LDS_KEYS candidates; the
CCM_OCT_REG_KEYS=0 switch), trees that stop at the roots, in a full pass or in the careful pass, empty and one-key levels, and the
per-frame strides of a batch on one lane and on two."""
import os
import subprocess
import sys

import numpy as np
import pytest

import octree_stage_ref as S
from motioncheck_ccm_slam_amd.orb import ORBextractor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(ctx, oracle, imgs, nfeatures=1000):
    ex = ORBextractor(nfeatures, 1.2, 8, 20, 7, ctx=ctx)
    kps, desc, counts = ex.extract_batch(imgs)
    par = oracle.default_params(nfeatures, 1.2, 8, 20, 7)
    return S.check_stage(ex, oracle, par, kps, counts, imgs.shape[2], imgs.shape[1])


def test_a_bench_frame(ctx, oracle):
    """752x480, 1000 features: level 0 has more cells than one round of the loop gather, its tree ends in the careful pass; the top
    levels have fewer than 64 cells."""
    info = _run(ctx, oracle, S.frame_a()[None])
    assert info[(0, 0)]["cells"] > S.GATHER_ROUND
    assert info[(0, 0)]["n"] > info[(0, 0)]["quota"] and info[(0, 0)]["selected"] >= info[(0, 0)]["quota"]      # the careful pass was reached
    assert 0 < info[(0, 7)]["cells"] < 64 and 0 < info[(0, 6)]["cells"] < 64


def test_b_small_quota(ctx, oracle):
    """the same frame, 60 features: quotas 13 ... 4 (the reference's table gives the top level 4, above the two roots of 752x480), so a
    tree is in its careful pass one division behind the roots.  16 features as well: quotas 3 ... 1, at or below the number of roots
    -- trees that stop at the roots -- and a node list so short (16 slots) that its LDS cannot hold the cell offsets of the lower
    levels: those take the loop gather, the top ones the one-trip form."""
    info = _run(ctx, oracle, S.frame_a()[None], nfeatures=60)
    assert info[(0, 7)]["quota"] <= 4 * 2 and info[(0, 7)]["n"] > info[(0, 7)]["quota"]      # 752x480: two roots
    info = _run(ctx, oracle, S.frame_a()[None], nfeatures=16)
    assert info[(0, 7)]["quota"] <= 2 and info[(0, 7)]["n"] > 2 and info[(0, 0)]["cells"] > 5 * 16 > info[(0, 7)]["cells"]


def test_c_four_roots(ctx, oracle):
    """1241x376, 1500 features: four roots, 440 cells on level 0"""
    from motioncheck_ccm_slam_amd import synth
    info = _run(ctx, oracle, synth.frame(42, 1241, 376, n_rect=990)[None], nfeatures=1500)
    assert info[(0, 0)]["cells"] > S.GATHER_ROUND and info[(0, 0)]["n"] > info[(0, 0)]["quota"]


def test_d_dense_corners(ctx, oracle):
    """seeded 2 px binary blocks at 320x240: a cell with more than 16 candidates on a level the one-trip gather takes, and a level
    with more than OCT_LDS_KEYS candidates (keys and node ids in global memory)"""
    info = _run(ctx, oracle, S.dense_frame(320, 240)[None])
    assert info[(0, 0)]["n"] <= S.OCT_LDS_KEYS and info[(0, 0)]["max_cell"] > 16
    assert max(info[(0, l)]["n"] for l in range(8)) > S.OCT_LDS_KEYS


def test_e_empty_and_single(ctx, oracle):
    info = _run(ctx, oracle, np.stack([S.blank_frame(320, 240), S.one_corner_frame(320, 240)]))
    assert all(info[(0, l)]["n"] == 0 and info[(0, l)]["selected"] == 0 for l in range(8))
    # (the step edge itself is no FAST corner at full resolution: the resized levels bring the single candidates, and empty levels below)
    assert info[(1, 0)]["n"] == 0 and info[(1, 3)]["n"] == 1 and info[(1, 3)]["selected"] == 1 and info[(1, 7)]["n"] == 1


_CHILD = r'''
import sys
import numpy as np
import torch
torch.cuda.init()
import octree_stage_ref as S
from motioncheck_ccm_slam_amd import _lib
from motioncheck_ccm_slam_amd.orb import ORBextractor, lane_plan
from oracle import oracle_py as O
mode = sys.argv[1]
ctx = _lib.Context(0)
ex = ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx)
par = O.default_params()
if mode == "reg_keys_off":
    imgs = S.frame_a()[None]
    kps, desc, counts = ex.extract_batch(imgs)
else:
    imgs = np.stack([S.frame_a(), S.dense_frame(752, 480), S.blank_frame(752, 480)])
    dev = torch.from_numpy(imgs).cuda()
    ex.extract_dev(dev.data_ptr(), 752, 480, 752, 752 * 480, 3)
    kps, desc, counts = ex.fetch()
info = S.check_stage(ex, O, par, kps, counts, 752, 480)
if mode != "reg_keys_off":
    assert max(info[(1, l)]["n"] for l in range(8)) > S.OCT_LDS_KEYS and counts[2] == 0 and counts[0] > 900
print("ok")
'''


def _child(mode, env):
    out = subprocess.run([sys.executable, "-c", _CHILD, mode], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **env))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_f_keys_in_global_memory():
    """case A with CCM_OCT_REG_KEYS=0 (read once per process): every level takes the loop gather and keeps keys and node ids in global memory"""
    _child("reg_keys_off", {"CCM_OCT_REG_KEYS": "0"})


@pytest.mark.parametrize("lane_frames", ["0", "1"])
def test_g_three_frames(lane_frames):
    """the bench frame, a dense frame and a blank one in one device-resident call: per-frame strides of every array the kernel indexes;
    on one lane (CCM_ORB_LANE_FRAMES=0) and as three chunks on two lanes (=1: a value below the batch minimum lowers the minimum)"""
    from motioncheck_ccm_slam_amd.orb import lane_plan
    ex_out = 1000 + 4 * 8                      # any out_per_frame: the plan's chunk count for lane_frames 1 is the frame count
    assert len(lane_plan(3, ex_out, int(lane_frames))) == (3 if lane_frames == "1" else 1)
    _child("three_frames", {"CCM_ORB_LANE_FRAMES": lane_frames})
