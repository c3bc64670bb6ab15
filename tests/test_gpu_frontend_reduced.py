"""FrontendConfig::imdecode_reduce_ (IMREAD_REDUCED_GRAYSCALE_N) behind slam::Frontend and slam::FrontendGroup:
ObserveCompressedImage on JPEG payloads of twice the object's image size books the same problem (SerializeSLAMProblem, byte
for byte) as ObserveImage on the images the system's libjpeg decodes from them at 1/2 (tests/jpeg_ref_reduced.py); in a group
it is per camera -- a 320 x 240 camera at 2 and a 160 x 120 camera at 1 share one 160 x 120 context; a bayer_rggb8 frame at a
reduced size is refused and books nothing."""
import io
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

W, H, NF, LIFE, N = 160, 120, 500, 3, 6
F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
F_SHIFT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 1.5]], np.float32)
Q = (1.0, 0.0, 0.0, 0.0)


def _jpeg(img, i):
    import PIL.Image as PIL
    b = io.BytesIO()
    kw = [dict(quality=88), dict(quality=85, progressive=True), dict(quality=82, restart_marker_rows=2)][i % 3]
    PIL.fromarray(np.ascontiguousarray(img), "L").save(b, "JPEG", **kw)
    return b.getvalue()


@pytest.fixture(scope="module")
def cameras():
    """[camera 0: 320 x 240 files read at 1/2, camera 1: 160 x 120 files read whole] -> per camera (d, [(left file, right file)],
    [(left image, right image) as libjpeg decodes them at 1/d])."""
    import jpeg_ref_reduced as ref
    from vision_slam_frontend_amd import synth
    assert ref.available(), "no libjpeg.so.8 to build tests/cpp/jpeg_ref_reduced.c against"
    out = []
    for cam, d in enumerate((2, 1)):
        sc = synth.Scene(W * d, H * d, n_objects=400 * d, seed=synth.BASE_SEED + 31 * cam)
        files = [(_jpeg(sc.render(f, 0), f), _jpeg(sc.render(f, 1), f + 1)) for f in range(N)]
        images = []
        for pair in files:
            dec = [ref.imdecode_reduced_gray(x, d, W, H) for x in pair]
            assert all(st == 0 and warn == 0 for st, _, warn in dec)
            images.append((dec[0][1], dec[1][1]))
        out.append((d, files, images))
    return out


def _reference(images, F):
    from vision_slam_frontend_amd import frontend
    fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=F, best_percent=0.3, frame_life=LIFE)
    try:
        fe.observe_odometry((0.0, 0.0, 0.0), Q, -1.0)   # the first pose: OdomCheck compares the later ones with it
        for f, (left, right) in enumerate(images):
            fe.observe_odometry((0.3 * (f + 1), 0.0, 0.0), Q, float(f))
            assert fe.observe_image(left, right, f + 0.5)
        assert fe.num_poses == N
        return fe.serialize_problem()
    finally:
        fe.close()


@pytest.mark.parametrize("pipelined", [False, True])
def test_frontend_books_what_observe_image_books_on_the_library_images(cameras, pipelined):
    from vision_slam_frontend_amd import frontend
    d, files, images = cameras[0]
    want = _reference(images, F_RECT)
    assert len(want) > 6 * 20 * 28   # not trivial: six nodes of more than twenty 28-byte vision features each
    fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, best_percent=0.3, frame_life=LIFE, imdecode_reduce=d)
    try:
        fe.set_pipelined(pipelined)
        fe.observe_odometry((0.0, 0.0, 0.0), Q, -1.0)
        for f, (left, right) in enumerate(files):
            fe.observe_odometry((0.3 * (f + 1), 0.0, 0.0), Q, float(f))
            assert fe.observe_compressed_image(left, right, time=f + 0.5)
        assert fe.serialize_problem() == want and fe.refused_frames == 0
    finally:
        fe.close()


def test_group_takes_the_denominator_per_camera(cameras):
    from vision_slam_frontend_amd import frontend
    FS = [F_RECT, F_SHIFT]
    want = [_reference(cameras[m][2], FS[m]) for m in range(2)]
    assert want[0] != want[1]
    group = frontend.FrontendGroup(W, H, FS, nfeatures=NF, best_percents=[0.3, 0.3], frame_life=LIFE,
                                   imdecode_reduces=[cameras[0][0], cameras[1][0]])
    try:
        group.set_pipelined(True)
        group.set_queue(8, 4, 0)
        for m in range(2):
            group.observe_odometry(m, (0.0, 0.0, 0.0), Q, -1.0)
        for f in range(N):
            for m in (1, 0) if f % 2 else (0, 1):
                group.observe_odometry(m, (0.3 * (f + 1), 0.0, 0.0), Q, float(f))
                left, right = cameras[m][1][f]
                assert group.observe_compressed_image(m, left, right, time=f + 0.5)
        got = [group.serialize_problem(m) for m in range(2)]
        stats = group.queue_stats()
    finally:
        group.close()
    assert got == want
    assert stats["frames"] == 2 * N and stats["compressed"] == 2 * N and stats["reduced_frames"] == N


def test_bayer_at_a_reduced_size_is_refused_and_books_nothing(cameras):
    from vision_slam_frontend_amd import capi, frontend
    d, files, images = cameras[0]
    fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, best_percent=0.3, frame_life=LIFE, imdecode_reduce=2)
    ref = frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, best_percent=0.3, frame_life=LIFE, imdecode_reduce=2)
    try:
        for obj in (fe, ref):
            obj.observe_odometry((0.0, 0.0, 0.0), Q, -1.0)
        for f in range(2):
            for obj in (fe, ref):
                obj.observe_odometry((0.3 * (f + 1), 0.0, 0.0), Q, float(f))
            added = fe.observe_compressed_image(files[f][0], files[f][1], bayer_rggb8=True, time=f + 0.25,
                                                allow_status=(capi.VSF_ERR_INVALID_ARG,))
            assert not added and fe.last_status == capi.VSF_ERR_INVALID_ARG and fe.num_poses == f
            fe.set_imdecode_reduce(2)   # a valid setting right after a refusal: the refusal's status is not handed on
            assert fe.last_status == capi.VSF_OK
            assert fe.observe_compressed_image(files[f][0], files[f][1], time=f + 0.5)
            assert ref.observe_compressed_image(files[f][0], files[f][1], time=f + 0.5)
        assert fe.serialize_problem() == ref.serialize_problem() and fe.num_poses == 2
        with pytest.raises(capi.VsfError):
            fe.set_imdecode_reduce(3)
        # a PNG payload at a reduced size is refused too, by the queue's host half
        import PIL.Image as PIL
        b = io.BytesIO()
        PIL.fromarray(images[0][0], "L").save(b, "PNG")
        fe.observe_odometry((0.9, 0.0, 0.0), Q, 2.0)
        assert not fe.observe_compressed_image(b.getvalue(), b.getvalue(), time=2.5, allow_status=(capi.VSF_ERR_UNSUPPORTED,))
        assert fe.last_status == capi.VSF_ERR_UNSUPPORTED and fe.num_poses == 2
    finally:
        fe.close()
        ref.close()


def test_the_byte_cap_is_the_configurations_and_applies_to_the_file_as_it_is(cameras):
    """FrontendConfig::compressed_cap_: the default cap is sized by the REDUCED image, so a Frontend for a larger camera states
    its own.  One byte too few refuses the frame (VSF_ERR_CAPACITY, nothing booked); raised while nothing is in flight, the same
    frame is taken -- and a group's one cap is set through its constructor."""
    from vision_slam_frontend_amd import capi, frontend
    d, files, images = cameras[0]
    largest = max(len(f) for pair in files[:2] for f in pair)
    fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, best_percent=0.3, frame_life=LIFE, imdecode_reduce=d,
                           compressed_cap=largest - 1)
    try:
        fe.observe_odometry((0.0, 0.0, 0.0), Q, -1.0)
        fe.observe_odometry((0.3, 0.0, 0.0), Q, 0.0)
        assert not fe.observe_compressed_image(files[0][0], files[0][1], time=0.5, allow_status=(capi.VSF_ERR_CAPACITY,))
        assert fe.last_status == capi.VSF_ERR_CAPACITY and fe.num_poses == 0
        fe.set_compressed_cap(largest)
        assert fe.last_status == capi.VSF_OK
        assert fe.observe_compressed_image(files[0][0], files[0][1], time=0.5) and fe.num_poses == 1
    finally:
        fe.close()
    group = frontend.FrontendGroup(W, H, [F_RECT, F_SHIFT], nfeatures=NF, frame_life=LIFE, imdecode_reduces=[2, 1],
                                   compressed_cap=largest - 1)
    try:
        group.observe_odometry(0, (0.0, 0.0, 0.0), Q, -1.0)
        group.observe_odometry(0, (0.3, 0.0, 0.0), Q, 0.0)
        assert not group.observe_compressed_image(0, files[0][0], files[0][1], time=0.5, allow_status=(capi.VSF_ERR_CAPACITY,))
        group.members[1].set_compressed_cap(largest)   # (any member: the cap is the group's)
        assert group.observe_compressed_image(0, files[0][0], files[0][1], time=0.5)
        assert group.flush() and group.members[0].num_poses == 1
    finally:
        group.close()
