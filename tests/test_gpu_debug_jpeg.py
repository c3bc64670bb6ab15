"""vsf_observe_set_debug_jpeg: the queue's debug images leave as JPEG files.  Every frame's two files must be what
cv::imencode(".jpg") -- the system's libjpeg driven as OpenCV 3.2 drives it, tests/jpeg_enc_ref.py -- writes for the RAW canvases
an identical run with vsf_observe_set_debug_images alone returns; every result byte (header words 14 / 15 included) is unchanged; a
frame without an image has no file; with the switch off nothing more is launched than without the call.  Then the same bytes
through slam::Frontend in queued mode."""
import ctypes as C

import numpy as np
import pytest

import jpeg_enc_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not ref.available():
    pytest.skip("libjpeg.so.8 cannot be loaded", allow_module_level=True)

from debug_files_run import F_RECT, H, LIFE, NF, SEED, W, make_frames, run  # noqa: E402


@pytest.fixture(scope="module")
def frames():
    return make_frames()


def _run(frames, depth, images, jpeg):
    """jpeg: None = the call is never made.  -> (results, raw canvases or files per frame, stats)"""
    return run(frames, depth, images, "jpeg", jpeg)


@pytest.mark.parametrize("depth", [1, 4])
def test_files_equal_the_reference_encode_of_the_raw_canvases(frames, depth):
    raw_out, canvases, raw_stats = _run(frames, depth, True, None)
    jpg_out, files, stats = _run(frames, depth, True, 95)
    assert len(files) == len(canvases) == len(frames)
    # the shape of the raw run: the first frame has no match image, the frame with the empty right image no stereo image (nor has
    # the one behind it: its threshold is the NaN of a frame without stereo matches) -- and the others have both
    assert canvases[0][1] is None and canvases[2][0] is None
    assert canvases[0][0] is not None and canvases[4][0] is not None and all(c[1] is not None for c in canvases[1:])
    for i, ((cs, cm), (fs, fm)) in enumerate(zip(canvases, files)):
        assert (fs is None) == (cs is None) and (fm is None) == (cm is None), i
        if cs is not None:
            assert fs == ref.imencode(cs, 95), "stereo file of frame %d" % i
        if cm is not None:
            assert fm == ref.imencode(cm, 95), "match file of frame %d" % i
    for a, b in zip(raw_out, jpg_out):  # header words 14 / 15 and every other result byte
        assert a.tobytes() == b.tobytes()
    # ten launches per batch on top of the raw run's, which in turn has two copy commands per batch that this one has not
    assert stats["debug_jpeg_commands"] == 10 * stats["batches"] > 0
    assert sum(stats["launches"].values()) == sum(raw_stats["launches"].values()) + 8 * stats["batches"]


def test_the_switch_needs_the_images_and_costs_nothing_when_off(frames):
    from vision_slam_frontend_amd import capi
    L = capi.lib()
    with capi.Context(capi.default_params(W, H, max_images=2, nfeatures=NF), device=0) as ctx:
        assert L.vsf_observe_set_debug_jpeg(ctx._h, 95) == capi.VSF_ERR_INVALID_ARG  # nobody draws the images
        assert L.vsf_observe_set_debug_jpeg(ctx._h, 101) == capi.VSF_ERR_INVALID_ARG
        assert L.vsf_observe_set_debug_jpeg(ctx._h, 0) == capi.VSF_OK
    counted = ("frames", "batches", "max_batch", "solo", "forced", "depth", "bmax", "compressed", "ingest_commands",
               "compressed_bytes", "debug_jpeg_commands", "launches")  # launches: per stage, as vsf_profile_read counts them
    for images in (False, True):
        out_a, pics_a, st_a = _run(frames, 4, images, None)   # the parent's behaviour: the call is never made
        out_b, pics_b, st_b = _run(frames, 4, images, 0)      # ... and made with 0
        assert {k: st_a[k] for k in counted} == {k: st_b[k] for k in counted} and st_b["debug_jpeg_commands"] == 0
        assert [o.tobytes() for o in out_a] == [o.tobytes() for o in out_b]
        for (sa, ma), (sb, mb) in zip(pics_a, pics_b):
            assert (sa is None) == (sb is None) and (ma is None) == (mb is None)
            assert sa is None or np.array_equal(sa, sb)
            assert ma is None or np.array_equal(ma, mb)


def test_frontend_hands_out_the_same_files_in_queued_mode(frames):
    from vision_slam_frontend_amd import frontend
    _, canvases, _ = _run(frames, 4, True, None)
    C.CDLL("libc.so.6").srand(SEED)
    fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, frame_life=LIFE, debug_images=True, debug_jpeg_quality=95)
    fe.set_pipelined(True)
    fe.set_queue(depth=4)
    q = np.array([1, 0, 0, 0], np.float32)
    fe.observe_odometry([0, 0, 0], q, 1.0)
    assert fe.last_debug_image_compressed() is None and fe.last_debug_image_compressed(stereo=True) is None
    for f, (left, right) in enumerate(frames):
        fe.observe_odometry([0.3 * (f + 1), 0, 0], q, 10.0 + f)
        assert fe.observe_image(left, right) is True
    assert fe.num_poses == len(frames)
    assert fe.last_debug_image_compressed() == ref.imencode(canvases[-1][1], 95)
    assert fe.last_debug_image_compressed(stereo=True) == ref.imencode(canvases[-1][0], 95)
    fe.close()
