"""The one encode path behind vsf_jpeg_encode* / vsf_png_encode* and behind the queue's debug files, where the two formats meet:
one context's shared encoder scratch outgrown while an encode of the OTHER format is still queued, the shared staging of the
host-pointer calls, and one queue that hands out JPEG files, then PNG files, then raw canvases through two rebuilds.  Byte
equality against the system's libjpeg / libpng driven as OpenCV 3.2 drives them (tests/jpeg_enc_ref.py, tests/png_enc_ref.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import debug_files_run as dfr  # noqa: E402
import jpeg_enc_ref as jref  # noqa: E402
import png_enc_ref as pref  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not jref.available():
    pytest.skip("libjpeg.so.8 cannot be loaded", allow_module_level=True)
if not pref.available():
    pytest.skip("libpng16.so.16 cannot be loaded", allow_module_level=True)


def _images(n, w, h, ch, seed):
    """n different images: seeded noise and windows of a synthetic scene, alternating."""
    from vision_slam_frontend_amd import synth
    scene = synth.Scene(320, 240).render(seed % 5, 0)
    rng = np.random.default_rng(4000 + seed)
    out = []
    for i in range(n):
        if i & 1:
            out.append(rng.integers(0, 256, (h, w) if ch == 1 else (h, w, 3), dtype=np.uint8))
        else:
            win = [scene[20 + 9 * i + 5 * c:20 + 9 * i + 5 * c + h, 30 + 11 * i + 7 * c:30 + 11 * i + 7 * c + w] for c in range(ch)]
            out.append(np.ascontiguousarray(win[0] if ch == 1 else np.stack(win, -1)))
    assert len({o.tobytes() for o in out}) == n
    return out


def _reference(fmt, img, quality):
    return jref.imencode(img, quality) if fmt == "jpeg" else pref.imencode(img)


def test_shared_scratch_outgrown_while_the_other_format_is_still_queued():
    from vision_slam_frontend_amd import capi
    # (format, images, width, height, channels, quality): the scratch is built for the first, outgrown by far more than its quarter
    # of headroom by the second, outgrown again by the third while the second may still run in the retired buffer, and the fourth
    # runs inside a buffer far larger than its own layout
    steps = [("png", 2, 33, 31, 1, 0), ("jpeg", 6, 64, 48, 3, 50), ("png", 8, 64, 48, 3, 0), ("jpeg", 1, 7, 5, 1, 100)]
    with capi.Context(capi.default_params(320, 240, max_images=2, nfeatures=100), device=0) as ctx:
        jobs = []
        for k, (fmt, n, w, h, ch, q) in enumerate(steps):
            imgs = _images(n, w, h, ch, k)
            stride = capi.jpeg_encode_capacity(w, h, ch) if fmt == "jpeg" else capi.png_encode_capacity(w, h, ch)
            jobs.append((imgs, stride, torch.from_numpy(np.stack(imgs)).cuda(),
                         torch.full((n * stride,), 0x5A, dtype=torch.uint8, device="cuda"),
                         torch.full((n,), -7, dtype=torch.int32, device="cuda")))
        torch.cuda.synchronize()  # (the buffers are torch's; from here on NO synchronisation until every encode is queued)
        for (fmt, n, w, h, ch, q), (imgs, stride, d_src, d_out, d_n) in zip(steps, jobs):
            if fmt == "jpeg":
                ctx.jpeg_encode_batch_dev(d_src.data_ptr(), n, w, h, ch, w * h * ch, w * ch, q, d_out.data_ptr(), stride, d_n.data_ptr())
            else:
                ctx.png_encode_batch_dev(d_src.data_ptr(), n, w, h, ch, w * h * ch, w * ch, d_out.data_ptr(), stride, d_n.data_ptr())
        assert ctx.sync() == capi.VSF_OK
        files = 0
        for (fmt, n, w, h, ch, q), (imgs, stride, d_src, d_out, d_n) in zip(steps, jobs):
            out, nb = d_out.cpu().numpy().reshape(n, stride), d_n.cpu().numpy()
            for i, img in enumerate(imgs):
                want = _reference(fmt, img, q)
                assert nb[i] == len(want), (fmt, i, nb[i], len(want))
                assert out[i, :nb[i]].tobytes() == want, (fmt, i)
                files += 1
        assert files == 17
        # ... and the middle two through the host-pointer calls of the same context: their ONE staging buffer, grown between them
        assert ctx.jpeg_encode(jobs[1][0], quality=50) == [jref.imencode(i, 50) for i in jobs[1][0]]
        assert ctx.png_encode(jobs[2][0]) == [pref.imencode(i) for i in jobs[2][0]]
        assert ctx.sync() == capi.VSF_OK


def test_one_context_hands_out_both_forms_one_after_the_other():
    from vision_slam_frontend_amd import capi
    frames, depth = dfr.make_frames()[:3], 4
    _, canvases, _ = dfr.run(frames, depth, True, "png", None)  # the raw run, a context of its own
    L = capi.lib()
    with capi.Context(capi.default_params(dfr.W, dfr.H, max_images=2 * depth, nfeatures=dfr.NF), device=0) as ctx:
        ctx.observe_configure(depth=depth)
        dfr.seed(ctx)
        assert L.vsf_observe_set_debug_images(ctx._h, 1) == capi.VSF_OK
        assert L.vsf_observe_set_debug_jpeg(ctx._h, 90) == capi.VSF_OK
        _, files = dfr.submit_collect(ctx, frames, depth, "jpeg")
        assert len(files) == len(canvases) == 3
        for (cs, cm), (fs, fm) in zip(canvases, files):
            assert fs == (None if cs is None else jref.imencode(cs, 90))
            assert fm == (None if cm is None else jref.imencode(cm, 90))
        # the other form, on the same context: the queue is rebuilt for ONE (kind, quality)
        ctx.observe_reset()
        assert L.vsf_observe_set_debug_jpeg(ctx._h, 0) == capi.VSF_OK
        assert L.vsf_observe_set_debug_png(ctx._h, 1) == capi.VSF_OK
        dfr.seed(ctx)
        before = ctx.observe_stats()
        _, files = dfr.submit_collect(ctx, frames, depth, "png")  # (asserts that vsf_observe_debug_jpeg_view now refuses)
        after = ctx.observe_stats()
        for (cs, cm), (fs, fm) in zip(canvases, files):
            assert fs == (None if cs is None else pref.imencode(cs))
            assert fm == (None if cm is None else pref.imencode(cm))
        batches = after["batches"] - before["batches"]
        assert batches > 0 and after["debug_jpeg_commands"] - before["debug_jpeg_commands"] == 20 * batches
        # ... and none: the raw canvases again
        ctx.observe_reset()
        assert L.vsf_observe_set_debug_png(ctx._h, 0) == capi.VSF_OK
        dfr.seed(ctx)
        _, raw = dfr.submit_collect(ctx, frames, depth, None)  # (asserts that vsf_observe_debug_png_view is refused)
        for (cs, cm), (rs, rm) in zip(canvases, raw):
            assert (rs is None) == (cs is None) and (rm is None) == (cm is None)
            assert cs is None or np.array_equal(rs, cs)
            assert cm is None or np.array_equal(rm, cm)
        assert ctx.observe_stats()["debug_jpeg_commands"] == 0
