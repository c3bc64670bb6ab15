"""vsf_world_points_batch_dev (csrc/k_cloud.hip): the RViz point cloud of the reference's driver (AddFeaturePoints,
slam_frontend_main.cc:155-173) on synthetic vsf_vision_feature records, no images.

membership  exact, on the table of the issue: NaN / +-inf in each coordinate, (0,0,0), z = 0.1f (passes: (double)0.1f > 0.1)
            and the float below it, norm exactly 0.5 and 20.0 (both fail) with their float neighbours on each side, negative z
            with a large norm -- under the identity and under a non-trivial pose
counts      0, 1, 63, 64, 65, 129 and max_keypoints features in ONE call of seven frames with seven poses (one frame passes
            everything, one nothing, one alternates); the order is the feature order; the poison written into d_points
            beforehand survives behind d_npoints[f]; a call of 65 frames takes the second launch (64 transforms ride in one
            launch's arguments)
coordinates against a float64 evaluation of the same formula: |delta| <= 1e-5 (|loc| + |t_cam| + |p|) per coordinate, the
            project's 1e-5 measure for point3d (the float chain is ~20 roundings of 2^-24: ~1.2e-6 of those magnitudes)
restatement the device's bytes equal those of the host library's AddFeaturePoints (host/slam_visualization.h through ctypes),
            which compiles the same csrc/vsf_world_points.h"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = 300  # max_keypoints of the test's context
COUNTS = (0, 1, 63, 64, 65, 129, K)
POISON = 0xA5
# FrontendConfig::left_cam_to_robot (slam_frontend.cc:613-618)
CAM = np.float32([[0.009916590468, -0.2835522866, 0.9589055021, -0.01], [-0.9998698619, -0.01501486552, 0.005900269087, 0.06],
                  [0.01272480238, -0.9588392225, -0.2836642819, 0.53]])
IDENTITY = np.eye(3, 4, dtype=np.float32)


def _unit(q):
    q = np.float64(q)
    return np.float32(q / np.linalg.norm(q))


# loc xyz + quaternion xyzw
POSES = np.float32([
    [0, 0, 0, 0, 0, 0, 1],
    [1.5, -2.25, 0.5, *_unit([0, 0, 1, 1])],
    [-7.0, 3.0, 0.125, *_unit([1, 2, 3, 4])],
    [12.5, 0.75, -1.0, *_unit([-1, 0.5, 0.25, 2])],
    [0.3, 0.6, 0.9, *_unit([0.1, -0.2, 0.3, -0.9])],
    [-3.0, -4.0, 5.0, *_unit([1, 0, 0, 0])],
    [100.0, -50.0, 2.0, *_unit([0.5, 0.5, -0.5, 0.5])],
])


def _table():
    """(point3d, keep) rows of the membership table."""
    f = np.float32
    inf, nan = f(np.inf), f(np.nan)
    up = lambda v, to: np.nextafter(f(v), f(to))  # noqa: E731
    rows = []
    for bad in (nan, inf, -inf):
        for c in range(3):
            p = [f(1), f(1), f(1)]
            p[c] = bad
            rows.append((p, False))
    rows += [
        ([0, 0, 0], False),
        ([0, 0.6, f(0.1)], True), ([0, 0.6, up(0.1, 0)], False),
        ([0, 0, 0.5], False), ([0, 0, up(0.5, 1)], True), ([0, 0, up(0.5, 0)], False),
        ([0, 0, 20.0], False), ([0, 0, up(20.0, 0)], True), ([0, 0, up(20.0, 21)], False),
        ([12, 0, 16], False),  # 144 + 256 = 400 exactly: norm 20
        ([0.5, 0, f(0.1)], True),  # 0.25 + 0.1f^2 > 0.25: norm above 0.5
        ([1.5, 0, 2], True), ([3, 4, -5], False), ([-30, 40, -0.5], False), ([5, 5, 0.05], False), ([-3, 2, 6], True),
    ]
    return np.float32([r[0] for r in rows]), np.array([r[1] for r in rows])


def _records(points):
    from vision_slam_frontend_amd import capi
    r = np.zeros(len(points), capi.VISION_FEATURE_DTYPE)
    r["feature_idx"] = np.arange(len(points))
    r["pixel"] = 1.0
    r["point3d"] = points
    return r


def _reference64(pose, cam, p):
    """M * p in float64, M = (Translation(loc) * R(quat)) * cam."""
    loc, (x, y, z, w) = np.float64(pose[:3]), np.float64(pose[3:])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    c = np.float64(cam)
    pr = np.float64(p) @ c[:, :3].T + c[:, 3]
    return pr @ R.T + loc


def _bound(pose, cam, p):
    return 1e-5 * (np.linalg.norm(np.float64(pose[:3])) + np.linalg.norm(np.float64(cam)[:, 3]) +
                   np.linalg.norm(np.float64(p), axis=1))[:, None]


def _keep(p):
    """The predicate as the issue states it, on float32 inputs (norm: float sqrt of the float sum of squares)."""
    p = np.float32(p)
    with np.errstate(all="ignore"):
        norm = np.sqrt(np.float32(np.float32(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]), dtype=np.float32)
        z64, norm64 = p[:, 2].astype(np.float64), norm.astype(np.float64)
        return np.isfinite(p).all(axis=1) & (z64 > 0.1) & (norm64 > 0.5) & (norm64 < 20.0)


def _run(ctx, frames, poses, cam):
    """frames: list of (n_f, 3) float32 point arrays.  Returns (points [F][K][3] float64 incl. the poison, npoints [F])."""
    F = len(frames)
    from vision_slam_frontend_amd import capi
    rec = np.zeros((F, K), capi.VISION_FEATURE_DTYPE)
    rec["point3d"] = 7.0  # (rows behind a frame's count would pass the predicate: they must not be read)
    for f, p in enumerate(frames):
        rec[f, :len(p)] = _records(p)
    n = np.int32([len(p) for p in frames])
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(F, -1)).cuda()
    d_n = torch.from_numpy(n).cuda()
    d_pts = torch.full((F, K, 24), POISON, dtype=torch.uint8, device="cuda")
    d_np = torch.full((F,), -12345, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.world_points_batch_dev(d_rec.data_ptr(), d_n.data_ptr(), F, poses, cam, d_pts.data_ptr(), d_np.data_ptr())
    assert ctx.sync() == 0
    return d_pts.cpu().numpy().view(np.float64).reshape(F, K, 3), d_np.cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    from vision_slam_frontend_amd import capi
    with capi.Context(capi.default_params(320, 240, max_images=2, nfeatures=100, max_keypoints=K), device=0) as c:
        yield c


@pytest.fixture(scope="module")
def counts_case(ctx):
    """Seven frames of COUNTS features under seven poses, run ONCE: frame 3 (64) passes everything, frame 4 (65) nothing,
    frame 5 (129) alternates, the others are a seeded mix."""
    rng = np.random.default_rng(11)
    frames = []
    for f, n in enumerate(COUNTS):
        good = np.float32(rng.uniform(-6, 6, (n, 3)))
        good[:, 2] = np.abs(good[:, 2]) + 0.75  # z > 0.1, 0.75 <= norm < 20
        bad = np.float32(rng.uniform(-6, 6, (n, 3)))
        bad[:, 2] = -np.abs(bad[:, 2])
        bad[::3] = 0  # (quirk Q5's zero points among them)
        bad[1::7, 0] = np.nan
        pick = {3: np.ones(n, bool), 4: np.zeros(n, bool), 5: np.arange(n) % 2 == 0}.get(f, rng.random(n) < 0.6)
        frames.append(np.where(pick[:, None], good, bad).astype(np.float32))
    pts, npts = _run(ctx, frames, POSES, CAM)
    return frames, pts, npts


def test_membership_table_is_exact_under_two_poses(ctx):
    from vision_slam_frontend_amd import frontend
    table, keep = _table()
    assert np.array_equal(_keep(table), keep)  # (the table says what the issue's predicate says)
    poses = POSES[[0, 2]]
    for cam in (IDENTITY, CAM):
        pts, npts = _run(ctx, [table, table], poses, cam)
        for f in range(2):
            assert npts[f] == keep.sum()
            got = pts[f, :npts[f]]
            want = _reference64(poses[f], cam, table[keep])
            assert (np.abs(got - want) <= _bound(poses[f], cam, table[keep])).all()
            if f == 0 and cam is IDENTITY:
                assert np.array_equal(got, np.float64(table[keep]))  # the identity is exact: the kept rows, in feature order
            cpu = frontend.add_feature_points(cam, poses[f, :3], poses[f, 3:], table)
            assert got.tobytes() == cpu.tobytes()
            assert (pts[f, npts[f]:].view(np.uint8) == POISON).all()


def test_counts_and_order_in_one_call_of_seven_frames(counts_case):
    frames, pts, npts = counts_case
    for f, p in enumerate(frames):
        keep = _keep(p)
        assert npts[f] == keep.sum(), (f, npts[f], keep.sum())
    assert npts[0] == 0 and npts[3] == 64 and npts[4] == 0 and npts[5] == 65 and 0 < npts[6] < K and npts[2] < 63
    # feature order: under pose 0 (the identity rotation, loc 0) the cloud of frame 0 ... is empty, so order is read from the
    # float64 reference of every frame: point k of the output is kept feature k
    for f, p in enumerate(frames):
        keep = _keep(p)
        want = _reference64(POSES[f], CAM, p[keep])
        got = pts[f, :npts[f]]
        assert (np.abs(got - want) <= _bound(POSES[f], CAM, p[keep])).all(), f
        assert np.array_equal(np.float64(np.float32(got)), got)  # floats, widened


def test_nothing_is_written_behind_a_frames_count(counts_case):
    _, pts, npts = counts_case
    for f in range(len(COUNTS)):
        assert (pts[f, npts[f]:].view(np.uint8) == POISON).all(), f
    assert npts[6] < K  # (so that the largest frame has a tail to look at)


def test_device_equals_the_cpu_restatement_bit_for_bit(counts_case):
    from vision_slam_frontend_amd import frontend
    frames, pts, npts = counts_case
    for f, p in enumerate(frames):
        cpu = frontend.add_feature_points(CAM, POSES[f, :3], POSES[f, 3:], p)
        assert len(cpu) == npts[f] and pts[f, :npts[f]].tobytes() == cpu.tobytes(), f


def test_sixty_five_frames_take_a_second_launch(ctx):
    from vision_slam_frontend_amd import frontend
    rng = np.random.default_rng(5)
    F = 65
    frames = [np.float32(rng.uniform(-4, 4, (3 + f % 5, 3))) for f in range(F)]
    poses = np.float32([POSES[f % len(POSES)] for f in range(F)])
    poses[:, 0] += np.arange(F, dtype=np.float32)  # every frame its own transform
    pts, npts = _run(ctx, frames, poses, CAM)
    for f in (0, 1, 63, 64):
        cpu = frontend.add_feature_points(CAM, poses[f, :3], poses[f, 3:], frames[f])
        assert len(cpu) == npts[f] == _keep(frames[f]).sum() and pts[f, :npts[f]].tobytes() == cpu.tobytes(), f
        assert (pts[f, npts[f]:].view(np.uint8) == POISON).all()
    assert sum(npts) > F // 2


def test_the_host_pointer_call_and_refusals(ctx):
    from vision_slam_frontend_amd import capi
    table, keep = _table()
    got = ctx.world_points(_records(table), POSES[2], CAM)
    assert len(got) == keep.sum() and (np.abs(got - _reference64(POSES[2], CAM, table[keep])) <= _bound(POSES[2], CAM, table[keep])).all()
    assert len(ctx.world_points(_records(table[:0]), POSES[0], CAM)) == 0
    L = capi.lib()
    assert L.vsf_world_points_batch_dev(ctx._h, None, None, 1, None, None, None, None) == capi.VSF_ERR_INVALID_ARG
