"""The chunk plan of the extractor's two-lane device path (orb_lane_plan in csrc/orb_host.cpp, through ccm_orb_debug_lane_plan):
a pure function of the batch size, the geometry's keypoint slots per frame and the configured frames per chunk.  No GPU."""
import pytest

from motioncheck_ccm_slam_amd.orb import lane_plan

OUT_PER_FRAME = 1096                       # the bench geometry: 1000 features, 8 levels
# the batch at which orb_launch_orient_desc switches to eight slots per wave: out_per_frame * frames >= 4 * 8192
SWITCH_FRAMES = -(-4 * 8192 // OUT_PER_FRAME)
N_IMAGES = (1, 2, 29, 63, 64, 65, 255, 256, 1000)
LANE_FRAMES = (0, 1, 3, 32, 64, 128)


def test_the_switch_point_is_thirty_bench_frames():
    assert SWITCH_FRAMES == 30 and OUT_PER_FRAME * 29 < 4 * 8192 <= OUT_PER_FRAME * 30


@pytest.mark.parametrize("lane_frames", LANE_FRAMES)
@pytest.mark.parametrize("n", N_IMAGES)
def test_plan(n, lane_frames):
    plan = lane_plan(n, OUT_PER_FRAME, lane_frames)
    # exact cover, in order, no empty chunk
    assert plan and plan[0][0] == 0
    nxt = 0
    for f0, nrun, _lane in plan:
        assert f0 == nxt and nrun >= 1
        nxt = f0 + nrun
    assert nxt == n
    # alternating lanes, starting on the context's stream
    assert [lane for _, _, lane in plan] == [k & 1 for k in range(len(plan))]
    # sizes within one frame of each other, by the host-buffer path's even division
    sizes = [nrun for _, nrun, _ in plan]
    assert max(sizes) - min(sizes) <= 1
    assert [f0 for f0, _, _ in plan] == [n * k // len(plan) for k in range(len(plan))]
    # the minimum chunk: the descriptor kernel's switch point, unless the configured size itself is smaller
    minimum = min(SWITCH_FRAMES, lane_frames)
    if lane_frames == 0 or n < 2 * minimum or n <= lane_frames:
        assert plan == [(0, n, 0)]                   # one chunk on lane 0: the schedule without lanes
    else:
        assert len(plan) >= 2
        assert min(sizes) >= minimum
        assert len(plan) <= -(-n // lane_frames)     # never more chunks than the configured size asks for
    if lane_frames >= SWITCH_FRAMES:                 # the switch does not force a smaller chunk: every chunk of a split batch
        assert len(plan) == 1 or min(sizes) >= SWITCH_FRAMES      # runs the eight-slots-per-wave form


def test_known_plans():
    assert lane_plan(1, OUT_PER_FRAME, 128) == [(0, 1, 0)]                     # the single frame Tracking extracts
    assert lane_plan(256, OUT_PER_FRAME, 128) == [(0, 128, 0), (128, 128, 1)]
    assert lane_plan(256, OUT_PER_FRAME, 64) == [(0, 64, 0), (64, 64, 1), (128, 64, 0), (192, 64, 1)]
    assert lane_plan(65, OUT_PER_FRAME, 32) == [(0, 32, 0), (32, 33, 1)]       # three chunks of 21 or 22 would run the <1> form
    assert lane_plan(59, OUT_PER_FRAME, 32) == [(0, 59, 0)]
    assert lane_plan(7, OUT_PER_FRAME, 1) == [(k, 1, k & 1) for k in range(7)]
    assert lane_plan(7, OUT_PER_FRAME, 2) == [(0, 2, 0), (2, 2, 1), (4, 3, 0)]
    assert lane_plan(7, OUT_PER_FRAME, 3) == [(0, 3, 0), (3, 4, 1)]
    assert lane_plan(6, OUT_PER_FRAME, 2) == [(0, 2, 0), (2, 2, 1), (4, 2, 0)]
    # a geometry with few slots per frame needs more frames per chunk: 110 frames of 300 slots reach the switch point
    assert lane_plan(512, 300, 128) == [(0, 128, 0), (128, 128, 1), (256, 128, 0), (384, 128, 1)]
    assert lane_plan(400, 300, 128) == [(0, 133, 0), (133, 133, 1), (266, 134, 0)]     # four chunks of 100 would run the <1> form
    assert lane_plan(219, 300, 128) == [(0, 219, 0)]


def test_bad_arguments_are_refused():
    from motioncheck_ccm_slam_amd import _lib
    lib = _lib.load()
    assert lib.ccm_orb_debug_lane_plan(-1, OUT_PER_FRAME, 0, None, None, None, 0) == -1
    assert lib.ccm_orb_debug_lane_plan(4, 0, 0, None, None, None, 0) == -1
    assert lib.ccm_orb_debug_lane_plan(4, OUT_PER_FRAME, -1, None, None, None, 0) == -1
    assert lib.ccm_orb_debug_lane_plan(0, OUT_PER_FRAME, 8, None, None, None, 0) == 0
    assert lib.ccm_orb_debug_lane_plan(256, OUT_PER_FRAME, 64, None, None, None, 0) == 4      # the count alone
