"""The ONE decode path behind vsf_jpeg_decode_gray_batch, vsf_png_decode_gray_batch, vsf_imdecode_gray_batch and the
ObserveImage queue (decode_runs, vsf_ingest.hip): what a shared routine can get wrong that the per-decoder tests do not look
at -- where each run of one format starts inside the one upload, and decoder scratch that a call outgrows while the decode
of the call before it is still queued.  Expected bytes come from the system's libjpeg / libpng driven as cv::imdecode drives
them (tests/jpeg_ref.py, tests/png_ref.py); equality is byte for byte, so there is no tolerance to choose."""
import io
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

KINDS = ("baseline", "restart", "progressive", "gray_png", "rgb_png")


def _refs():
    import jpeg_ref
    import png_ref
    if not (jpeg_ref.available() and png_ref.available()):
        pytest.skip("the system's libjpeg / libpng are not loadable here")
    return jpeg_ref, png_ref


def _file(img, kind):
    Image = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    if kind == "rgb_png":
        Image.fromarray(np.dstack([img, np.roll(img, 3, 0), 255 - img]), "RGB").save(b, "PNG")
        return b.getvalue()
    im = Image.fromarray(np.ascontiguousarray(img), "L")
    if kind == "baseline":
        im.save(b, "JPEG", quality=88)
    elif kind == "restart":
        im.save(b, "JPEG", quality=82, restart_marker_rows=2)
    elif kind == "progressive":
        im.save(b, "JPEG", quality=85, progressive=True)
    else:
        im.save(b, "PNG", compress_level=4)
    return b.getvalue()


def _reference(data, w, h):
    jpeg_ref, png_ref = _refs()
    st, img, _ = (png_ref if data[:4] == b"\x89PNG" else jpeg_ref).imdecode_gray(data, w, h)
    assert st == 0 and img.shape == (h, w), st
    return img


def test_calls_that_outgrow_the_scratch_of_a_decode_still_queued():
    """Three calls on one context with NO sync between them, 64x48 files of all five kinds (baseline JPEG, JPEG with restart
    intervals, progressive JPEG, gray PNG, RGB PNG), a different image per file:
      1. imdecode of (baseline, gray PNG): the scratch is built for one file of each decoder;
      2. imdecode of twelve files whose runs of one format have one or two files -- two baseline files (the parallel decoder's
         streams and coefficients for two: more than the quarter of headroom), a colour + a gray PNG (the scanlines and the
         per-file words of two), a lone progressive file (its flags and Huffman tables: new), a progressive + a restart file
         (the pipelined and the one-wave decoder in one run) -- so both JPEG decoders, the progressive path and both PNG
         kernels run out of scratch that was grown while call 1's decode may still be using the outgrown buffers;
      3. the three JPEG kinds alone through vsf_jpeg_decode_gray_batch.
    Then ONE sync returns VSF_OK and every image of the three destinations equals libjpeg's / libpng's."""
    torch = pytest.importorskip("torch")
    from vision_slam_frontend_amd import capi, synth
    w, h = 64, 48
    calls = [("baseline", "gray_png"),
             ("baseline", "gray_png", "baseline", "baseline", "rgb_png", "gray_png", "progressive", "rgb_png", "restart",
              "gray_png", "progressive", "restart"),
             ("baseline", "restart", "progressive")]
    assert set(calls[1]) == set(KINDS)
    seed = iter(range(100))
    files = [[_file(synth.stereo_pair(w, h, next(seed), n_objects=30)[0], k) for k in kinds] for kinds in calls]
    want = [np.stack([_reference(f, w, h) for f in fs]) for fs in files]
    dev = torch.device("cuda", 0)
    dst = [torch.full((len(fs), h, w), 0xA5, dtype=torch.uint8, device=dev) for fs in files]
    torch.cuda.synchronize()
    with capi.Context(capi.default_params(320, 240, max_images=2, nfeatures=100)) as c:
        assert c.imdecode_gray_batch(files[0], w, h, dst[0].data_ptr(), w * h, w) == capi.VSF_OK
        assert c.imdecode_gray_batch(files[1], w, h, dst[1].data_ptr(), w * h, w) == capi.VSF_OK
        assert c.jpeg_decode_gray_batch(files[2], w, h, dst[2].data_ptr(), w * h, w) == capi.VSF_OK
        assert c.sync() == capi.VSF_OK
        for k, (d, ref) in enumerate(zip(dst, want)):
            got = d.cpu().numpy()
            for i in range(len(ref)):
                np.testing.assert_array_equal(got[i], ref[i], err_msg="call %d file %d (%s)" % (k + 1, i, calls[k][i]))


def test_one_batch_of_the_queue_with_runs_of_every_length():
    """The same through the queue, at the 320x240 of tests/test_gpu_observe_compressed.py (whose helpers run it): depth 4,
    min_batch 4, so the four frames (baseline, RGB PNG), raw, (progressive, restart), (gray PNG, gray PNG) are ONE batch whose
    eight images hold four runs -- JPEG 1, PNG 1, [raw, raw], JPEG 2, PNG 2 -- at four offsets of one upload.  The results equal
    those of the reference-decoded images submitted raw, and the compressed path issued 1 upload + 4 runs + the finish."""
    import test_gpu_observe_compressed as oc
    frames = oc._scene_frames(4)
    kinds = [("baseline", "rgb_png"), None, ("progressive", "restart"), ("gray_png", "gray_png")]
    spec = [("raw", left, right) if k is None else ("cmp", _file(left, k[0]), _file(right, k[1]))
            for (left, right), k in zip(frames, kinds)]
    calib = oc._calib()

    def run(spec):
        with oc._context(4, min_batch=4) as ctx:
            ctx.observe_set_compressed_cap(1 << 20)  # (a colour PNG of a noisy scene is larger than the default, width x height + 64 KB)
            tickets = []
            for kind, left, right in spec:  # the fourth submit releases the batch
                if kind == "raw":
                    tickets.append(ctx.observe_submit(left, right, calib, best_percent=oc.BP, frame_life=oc.LIFE))
                else:
                    tickets.append(ctx.observe_submit_compressed(left, right, calib, best_percent=oc.BP, frame_life=oc.LIFE)[1])
            return [ctx.observe_collect_bytes(t, oc.LIFE) for t in tickets], ctx.observe_stats()

    got, stats = run(spec)
    want, _ = run(oc._reference_spec(spec, False))
    oc._assert_equal_runs(got, want)
    assert (stats["frames"], stats["batches"], stats["max_batch"], stats["compressed"]) == (4, 1, 4, 3)
    assert stats["ingest_commands"] == 1 + 4 + 1
    assert all(int(b[52:56].view(np.uint32)[0]) == 0 for _, b in got)
