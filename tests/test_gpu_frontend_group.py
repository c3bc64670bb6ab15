"""slam::FrontendGroup: three Frontend configurations with different calibrations on ONE context and ONE ObserveImage queue
(member i is stream i of vsf_observe_set_streams), odometry and images interleaved, pipelined at depth 16.  Each member's
SerializeSLAMProblem equals, byte for byte, that of a separate synchronous Frontend fed the same calls."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, NF, LIFE, N = 320, 240, 700, 3, 8
F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
F_SHIFT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 1.5]], np.float32)
F_DENSE = np.array([[2.31e-08, -1.17e-05, 3.45e-03], [1.22e-05, 9.8e-08, -0.11], [-4.1e-03, 0.108, 1.0]], np.float32)
FS = [F_RECT, F_SHIFT, F_DENSE]
BPS = [0.3, 0.6, 0.3]
ORDER = [0, 0, 0, 1, 0, 1, 1, 1, 0, 2, 2, 1, 2, 2, 2, 0, 1, 2, 0, 1, 2, 2, 0, 1]  # runs of one member; member 2 starts late
Q = (1.0, 0.0, 0.0, 0.0)


def _calls():
    """The driver's calls, in order: ("odom", member, translation, time) / ("image", member, left, right, time).  Every member
    moves 0.3 m per frame (min_odom_translation is 0.2) -- except once, where it has not moved: OdomCheck gates that frame (no
    node, nothing submitted)."""
    from vision_slam_frontend_amd import synth
    scenes = [synth.Scene(W, H, n_objects=400, seed=synth.BASE_SEED + 17 * m) for m in range(3)]
    calls, k = [], [0, 0, 0]
    for m in (2, 0, 1):  # the first pose of every member (OdomCheck compares the later ones with it)
        calls.append(("odom", m, (0.05 * m, 0.0, 0.0), 10.0 * m - 1.0))
    for step, m in enumerate(ORDER):
        f = k[m]
        k[m] += 1
        gated = (m, f) == (1, 4)
        x = 0.3 * (f if gated else f + 1) + 0.05 * m
        calls.append(("odom", m, (x, 0.0, 0.0), 10.0 * m + f))
        if step % 5 == 2:  # a second pose before the image: the frame is booked with the one its call saw
            calls.append(("odom", m, (x + 0.001, 0.0, 0.0), 10.0 * m + f + 0.5))
        calls.append(("image", m, scenes[m].render(f, 0), scenes[m].render(f, 1), 10.0 * m + f + 0.75))
    return calls


@pytest.mark.parametrize("thread", [0, 1])
def test_group_members_equal_separate_frontends(thread):
    from vision_slam_frontend_amd import frontend
    calls = _calls()
    want, want_added = [], [[], [], []]
    for m in range(3):
        fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=FS[m], best_percent=BPS[m], frame_life=LIFE)
        try:
            for c in calls:
                if c[1] != m:
                    continue
                if c[0] == "odom":
                    fe.observe_odometry(c[2], Q, c[3])
                else:
                    want_added[m].append(fe.observe_image(c[2], c[3], c[4]))
            want.append(fe.serialize_problem())
            assert fe.num_poses == N - (1 if m == 1 else 0)
        finally:
            fe.close()
    assert len(set(want)) == 3 and min(len(w) for w in want) > 10000

    group = frontend.FrontendGroup(W, H, FS, nfeatures=NF, best_percents=BPS, frame_life=LIFE)
    try:
        group.set_pipelined(True)
        group.set_queue(16, 8, 0)
        group.set_queue_thread(bool(thread))
        got_added = [[], [], []]
        for step, c in enumerate(calls):
            if c[0] == "odom":
                group.observe_odometry(c[1], c[2], Q, c[3])
            else:
                got_added[c[1]].append(group.observe_image(c[1], c[2], c[3], c[4]))
            if step == 40:  # reading one member's problem in the middle books everything in flight, in ticket order
                assert len(group.serialize_problem(2)) > 0
        got = [group.serialize_problem(m) for m in range(3)]
        stats = group.queue_stats()
        # the members themselves are Frontends: the same problem through the member's own view
        assert [m.serialize_problem() for m in group.members] == got
        assert [m.num_poses for m in group.members] == [N, N - 1, N]
    finally:
        group.close()
    assert got_added == want_added and want_added[1].count(False) == 1
    for m in range(3):
        assert got[m] == want[m], "member %d differs from a Frontend of its own" % m
    assert stats["streams"] == 3 and stats["frames"] == 3 * N - 1 and stats["depth"] == 16
