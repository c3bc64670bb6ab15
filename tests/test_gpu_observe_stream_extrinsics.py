"""A left_cam_to_robot per stream of the ObserveImage queue (vsf_observe_set_stream_cam_to_robot): two cameras on one robot
share a queue and each ticket's points equal, bit for bit, those of a one-stream context built with that camera's matrix
(the rectified rig of tests/test_gpu_observe_world_points.py, so the clouds are not empty); NULL returns a stream to the
context's matrix; the override survives vsf_observe_reset_stream and vsf_observe_reset and goes with another number of
streams."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import test_gpu_observe_world_points as wp  # noqa: E402

pytestmark = pytest.mark.gpu

LIFE, BP, NFR = wp.LIFE, wp.BP, 6
# the second camera: looks the other way, sits elsewhere on the robot
CAM_B = np.float32([[-0.0099, 0.2836, -0.9589, 0.21], [0.9999, 0.0150, -0.0059, -0.06], [0.0127, -0.9588, -0.2837, 0.47]])
CAMS = [wp.CAM, CAM_B]


def _frames():
    from vision_slam_frontend_amd import synth
    sc = synth.Scene(wp.W, wp.H, n_objects=400, seed=synth.BASE_SEED)
    return [(sc.render(f, 0), sc.render(f, 1)) for f in range(NFR)]


def _own_context(frames, cam, who, first=0):
    """THE reference: a one-stream context whose queue is built with `cam`; frame i carries wp._pose(first + i, who).
    -> per frame (result bytes, the points' bytes)"""
    calib, out = wp._calib(), []
    with wp._context(1, cloud=False) as ctx:
        ctx.observe_set_world_points(True, cam)
        for i, (left, right) in enumerate(frames):
            pose = wp._pose(first + i, who)
            ctx.observe_set_pose(0, pose[:3], pose[3:])
            t = ctx.observe_submit(left, right, calib, best_percent=BP, frame_life=LIFE)
            out.append((ctx.observe_collect_bytes(t, LIFE)[1].tobytes(), ctx.observe_world_points(t).tobytes()))
    return out


@pytest.fixture(scope="module")
def world():
    frames = _frames()
    want = {(who, c): _own_context(frames, CAMS[c], who) for who in (0, 1) for c in (0, 1)}
    assert all(len(w[1]) > 10 * 24 for w in want[0, 0]) and want[0, 0][1][1] != want[0, 1][1][1]
    return frames, want


def _run(ctx, frames, depth, streams=(0, 1), first=0):
    """Frames round-robin over `streams`, stream s with the poses of sequence s; -> per stream [(result, points)]."""
    calib, got, tickets = wp._calib(), {s: [] for s in streams}, []

    def collect():
        t, s = tickets.pop(0)
        got[s].append((ctx.observe_collect_bytes(t, LIFE)[1].tobytes(), ctx.observe_world_points(t).tobytes()))

    for i, (left, right) in enumerate(frames):
        for s in streams:
            if len(tickets) == depth:
                collect()
            pose = wp._pose(first + i, s)
            ctx.observe_set_pose(s, pose[:3], pose[3:])
            tickets.append((ctx.observe_submit_stream(s, left, right, calib, best_percent=BP, frame_life=LIFE), s))
    while tickets:
        collect()
    return got


@pytest.mark.parametrize("depth", [1, 4, 32])
def test_two_cameras_one_queue(world, depth):
    """Stream 0 keeps the context's matrix, stream 1 has its own: each ticket's points are its own context's."""
    frames, want = world
    with wp._context(depth, streams=2) as ctx:
        ctx.observe_set_stream_cam_to_robot(1, CAM_B)
        got = _run(ctx, frames, depth)
        stats = ctx.observe_stats()
    assert got[0] == want[0, 0] and got[1] == want[1, 1]
    assert stats["world_points_frames"] == 2 * NFR and (depth == 1 or stats["multi_stream_batches"] >= 1)


def test_null_reset_and_the_rules(world):
    """Both streams overridden (the context's matrix is then never read); NULL returns a stream to the context's; the
    override survives vsf_observe_reset_stream and vsf_observe_reset, and goes when the number of streams changes; a stream
    out of range is refused."""
    from vision_slam_frontend_amd import capi
    frames, want = world
    INV = capi.VSF_ERR_INVALID_ARG
    with wp._context(8, streams=2) as ctx:
        for bad in (-1, 2, 64):
            assert ctx.observe_set_stream_cam_to_robot(bad, CAM_B, allow_status=(INV,)) == INV
        ctx.observe_set_stream_cam_to_robot(0, CAM_B)
        ctx.observe_set_stream_cam_to_robot(1, wp.CAM)
        got = _run(ctx, frames[:3], 8)
        assert got[0] == want[0, 1][:3] and got[1] == want[1, 0][:3]
        # sticky and legal at any time: from here on stream 0 is the context's camera again, stream 1 the other one
        ctx.observe_set_stream_cam_to_robot(0, None)
        ctx.observe_set_stream_cam_to_robot(1, CAM_B)
        got = _run(ctx, frames[3:], 8, first=3)
        assert got[0] == want[0, 0][3:] and got[1] == want[1, 1][3:]
        # vsf_observe_reset_stream: a fresh window and the identity pose, the camera stays
        ctx.observe_reset_stream(1)
        got = _run(ctx, frames[:2], 8, streams=(1,))
        assert got[1] == want[1, 1][:2]
        # vsf_observe_reset: the queue goes, the camera stays
        ctx.observe_reset()
        got = _run(ctx, frames[:2], 8)
        assert got[0] == want[0, 0][:2] and got[1] == want[1, 1][:2]
        # another number of streams: other cameras
        ctx.observe_set_streams(3)
        got = _run(ctx, frames[:2], 8, streams=(1,))
        assert got[1] == want[1, 0][:2]


def test_a_group_of_two_cameras_keeps_two_clouds():
    """slam::FrontendGroup: two members that differ in left_cam_to_robot, visualization on -- each member's cloud and markers
    are those of a single Frontend with that matrix, and the two clouds differ although the cameras see the same frames."""
    from vision_slam_frontend_amd import frontend
    import test_gpu_frontend_visualization as fv
    frames = fv._frames(0)[:6]

    def drive(observe_odometry, observe_image):
        observe_odometry([0, 0, 0], [1, 0, 0, 0], 0.0)
        for f, (left, right) in enumerate(frames):
            t, q = fv._odometry(f)
            observe_odometry(t, q, 1.0 + f)
            assert observe_image(left, right) is True

    want = []
    for cam in CAMS:
        fe = frontend.Frontend(fv.W, fv.H, nfeatures=fv.NF, fundamental=fv.F_RECT, frame_life=fv.LIFE, cam_to_robot=cam,
                               visualization=True)
        try:
            fe.set_projections(fv.P_LEFT, fv.P_RIGHT)
            drive(fe.observe_odometry, fe.observe_image)
            assert fe.flush()
            want.append((fe.visualization()[0].tobytes(), fe.serialize_visualization(), fe.serialize_problem()))
        finally:
            fe.close()
    assert len(want[0][0]) > 24 * 50 and len(want[0][0]) == len(want[1][0]) and want[0][0] != want[1][0]
    group = frontend.FrontendGroup(fv.W, fv.H, [fv.F_RECT, fv.F_RECT], nfeatures=fv.NF, frame_life=fv.LIFE, cam_to_robots=CAMS,
                                   visualization=True)
    try:
        group.set_pipelined(True)
        group.set_queue(32, 4, 0)
        for m in group.members:
            m.set_projections(fv.P_LEFT, fv.P_RIGHT)
        for m in range(2):
            group.observe_odometry(m, [0, 0, 0], [1, 0, 0, 0], 0.0)
        for f, (left, right) in enumerate(frames):
            for m in range(2):
                t, q = fv._odometry(f)
                group.observe_odometry(m, t, q, 1.0 + f)
                assert group.observe_image(m, left, right) is True
        assert group.flush()
        got = [(group.members[m].visualization()[0].tobytes(), group.members[m].serialize_visualization(),
                group.serialize_problem(m)) for m in range(2)]
        assert group.queue_stats()["multi_stream_batches"] >= 1
    finally:
        group.close()
    for m in range(2):
        assert got[m] == want[m], "member %d differs from a Frontend of its own with its left_cam_to_robot" % m
