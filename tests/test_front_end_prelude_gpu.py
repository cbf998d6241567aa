"""What k_fast_cells and k_pyr_resize do before their first pixel load: k_fast_cells's argument block (the head's arguments in
front, level 0's image and the first frame as arguments of their own), the place of its status-word clear, the work order whose
grid sizes are explicit arguments, a call's later chunks (no clear, first frame > 0), and every head and border path of the
resize (two x-blocks with a nearly empty second, every width % 4, rows past the height inside a wave and a workgroup, idle
lanes, the single-frame upload).  Every case extracts a 2-frame batch (frame index > 0) unless it says otherwise and
compares exactly with the CPU oracle: the pyramid levels through the level tap, the FAST candidates of every level, keypoints and
descriptors.  The two switches that are read once per process (CCM_ORB_XCD, CCM_ORB_LANE_FRAMES) run in a child process each."""
import os
import subprocess
import sys

import numpy as np
import pytest

from motioncheck_ccm_slam_amd import _lib, synth
from motioncheck_ccm_slam_amd.orb import ORBextractor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NF, SF, INI, MN = 300, 1.2, 20, 7


def _pair(w, h, seed=7, n=2):
    return np.stack([synth.frame(seed + f, w, h, n_rect=max(60, 600 * w * h // (752 * 480))) for f in range(n)])


def _oracle_pyramid(O, img, nlevels):
    """The oracle's own chain of resizes (cv::resize INTER_LINEAR, bit-exact) from the frame."""
    par = O.default_params(NF, SF, nlevels, INI, MN)
    lw, lh = O.level_sizes(par, img.shape[1], img.shape[0])
    levels = [np.ascontiguousarray(img, np.uint8)]
    for l in range(1, nlevels):
        levels.append(O.resize(levels[-1], int(lw[l]), int(lh[l])))
    return levels


def _compare(O, ex, frames, nlevels, kps, desc, counts):
    """Levels, candidates of every level, keypoints and descriptors of the extractor's last call against the oracle."""
    par = O.default_params(NF, SF, nlevels, INI, MN)
    for f in range(len(frames)):
        want = _oracle_pyramid(O, frames[f], nlevels)
        for l in range(nlevels):
            got = ex.image_pyramid_level(f, l)
            assert got.shape == want[l].shape and (got == want[l]).all(), ("level", f, l)
            r = O.orb_extract(par, frames[f], cand_level=l)
            xy, sc = ex.fast_candidates(f, l)
            assert len(xy) == len(r["cand_xy"]) and (xy == r["cand_xy"]).all() and (sc == r["cand_score"]).all(), ("candidates", f, l)
        c = int(counts[f])
        assert c == len(r["kps"]), f
        for name in kps.dtype.names:
            assert (kps[f, :c][name] == r["kps"][name]).all(), (f, name)
        assert (desc[f, :c] == r["desc"]).all(), f


def _extract_dev(ctx, frames, nlevels, max_per_image=None):
    """frames [n, h, w] on the device, rows on dword boundaries (level 0 staged 16 bytes per lane), through the device entry point."""
    import torch
    n, h, w = frames.shape
    stride = (w + 3) & ~3
    host = np.zeros((n, h, stride), np.uint8)
    host[:, :, :w] = frames
    buf = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    ex = ORBextractor(NF, SF, nlevels, INI, MN, ctx=ctx, max_per_image=max_per_image)
    ex.extract_dev(buf.data_ptr(), w, h, stride, stride * h, n)
    return ex, buf


def _check(ctx, O, frames, nlevels):
    ex, buf = _extract_dev(ctx, frames, nlevels)
    kps, desc, counts = ex.fetch()
    _compare(O, ex, frames, nlevels, kps, desc, counts)
    del buf


def test_one_level_pyramid_opens_the_call(ctx, oracle):
    """nlevels = 1: no resize launch, k_fast_cells is the call's first kernel and clears the status word -- behind its pixel loads.
    The context has just extracted another geometry (three levels: another band table) and that call has LEFT the status word set
    (eight result rows for some hundred keypoints: CCM_E_CAPACITY), so a clear that did not happen shows as that error again.  Then
    the three-level geometry once more, whose first resize clears."""
    frames = _pair(182, 96)
    ex, buf = _extract_dev(ctx, frames, 3, max_per_image=8)
    with pytest.raises(_lib.CcmError) as e:
        ex.fetch()
    assert e.value.code == -4, e.value                  # CCM_E_CAPACITY
    del buf
    _check(ctx, oracle, frames, 1)
    ex, buf = _extract_dev(ctx, frames, 3, max_per_image=8)
    with pytest.raises(_lib.CcmError):
        ex.fetch()
    del buf
    _check(ctx, oracle, frames, 3)


CHILD = r'''
import sys
import numpy as np
import torch
torch.cuda.init()
sys.path.insert(0, sys.argv[1] + "/tests")
import test_front_end_prelude_gpu as T
from motioncheck_ccm_slam_amd import _lib
from oracle import oracle_py as O
ctx = _lib.Context(0)
frames = T._pair(182, 96)
T._check(ctx, O, frames, 3)
print("ok")
'''


def _child(**env):
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_xcd_work_order():
    """CCM_ORB_XCD=1: k_fast_cells deals its bands to the XCDs in contiguous ranges, from the grid sizes it now gets as explicit
    arguments (2 frames x 6 bands: the ranges are ragged)."""
    _child(CCM_ORB_XCD="1")


def test_later_chunk_of_a_call():
    """CCM_ORB_LANE_FRAMES=1 splits the 2-frame batch into the smallest two-chunk plan, [(0, 1, lane 0), (1, 1, lane 1)]: the second
    chunk's launches get no status word to clear and first frame 1."""
    from motioncheck_ccm_slam_amd.orb import lane_plan
    assert lane_plan(2, 300, 1) == [(0, 1, 0), (1, 1, 1)]       # (any out_per_frame: the switch point only matters above 1 frame per chunk)
    _child(CCM_ORB_LANE_FRAMES="1")


@pytest.mark.parametrize("w,h,nl", [
    (329, 91, 3), (330, 91, 3), (331, 91, 3), (332, 91, 3),     # level 1 is 274-277 wide: two x-blocks, the second nearly empty, every w % 4 in the last quad;
                                                                # 91, 76 and 63 rows: rows past the height inside a wave's 8 and a workgroup's 32
    (330, 96, 3),                                               # 96 and 80 rows: whole waves
    (96, 96, 2),                                                # a single x-block with idle lanes
])
def test_pyramid_levels_bit_for_bit(ctx, oracle, w, h, nl):
    if nl == 3 and h == 91:
        lw, lh = oracle.level_sizes(oracle.default_params(NF, SF, nl, INI, MN), w, h)
        assert int(lw[1]) == 274 + (w - 329) and (int(lh[1]), int(lh[2])) == (76, 63)
    _check(ctx, oracle, _pair(w, h, seed=3), nl)


def test_single_frame_host_call(ctx, oracle):
    """One frame from host memory: the aligned 2-D upload path, image stride 0."""
    frames = _pair(331, 91, seed=5, n=1)
    ex = ORBextractor(NF, SF, 3, INI, MN, ctx=ctx)
    kps, desc, counts = ex.extract_batch(frames)
    _compare(oracle, ex, frames, 3, kps, desc, counts)
