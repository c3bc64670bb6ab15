"""cv::imdecode(data, IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8) on the device (vsf_imdecode_reduced_gray_batch), bit for bit
against the system's libjpeg at scale 1/2, 1/4, 1/8 (tests/jpeg_ref_reduced.py): every file of tests/golden/jpeg -- baseline,
progressive, restart intervals and rows, 4:4:4 / 4:2:2 / 4:2:0, sizes from 1 x 1 to 320 x 240 --, through the parallel and
the one-wave decoder; files written from chosen coefficients (tests/jpeg_reduced_cases.py: single coefficients, the Huffman
limits under quantiser 255, cropped last blocks); one mixed batch per denominator with poisoned row padding; reduce = 1
against vsf_imdecode_gray_batch; a truncated file, which affects its own status alone; and the refusals."""
from pathlib import Path

import numpy as np
import pytest

import jpeg_reduced_cases as rc
import jpeg_ref_reduced as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLD = Path(__file__).resolve().parent / "golden" / "jpeg"
NAMES = sorted(np.load(GOLD / "expected_gray.npz").files)
POISON = 0xEE


@pytest.fixture(scope="module")
def ctxs():
    """[the default context, one whose JPEG files all take the one-wave decoder]"""
    from vision_slam_frontend_amd import capi
    a = capi.Context(capi.default_params(640, 480, max_images=2, nfeatures=500))
    b = capi.Context(capi.default_params(640, 480, max_images=2, nfeatures=500))
    b.debug_jpeg_serial(True)
    yield [a, b]
    a.close()
    b.close()


@pytest.fixture(scope="module")
def library():
    """{(name, d): libjpeg's pixels}, decoded once; every file here is read WITHOUT a warning (asserted), so every one is
    compared."""
    assert ref.available(), "no libjpeg.so.8 to build tests/cpp/jpeg_ref_reduced.c against"
    files = {n: (GOLD / (n + ".jpg")).read_bytes() for n in NAMES}
    files.update({"crafted_" + n: rc.write_file(c, q, w, h) for n, c, q, w, h in rc.cases()})
    want = {}
    for name, data in files.items():
        for d in (1, 2, 4, 8):
            st, img, warn = ref.imdecode_reduced_gray(data, d)
            assert st == 0 and warn == 0, (name, d, st, warn)
            want[(name, d)] = img
    return files, want


def _decode(ctx, files, d, w, h, extra=8, allow_status=()):
    from vision_slam_frontend_amd import capi
    pitch = (w + 3) // 4 * 4 + extra
    dst = torch.full((len(files), h, pitch), POISON, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    st = ctx.imdecode_reduced_gray_batch(files, d, w, h, dst.data_ptr(), h * pitch, pitch, allow_status=allow_status)
    if st != capi.VSF_OK:
        return st, None
    return ctx.sync(allow_capacity=True), dst.cpu().numpy()


def _check(got, want, label):
    h, w = want.shape
    np.testing.assert_array_equal(got[:, :w], want, err_msg=label)
    assert (got[:, w:] == POISON).all(), label + ": written beyond the row's last pixel"


@pytest.mark.parametrize("d", [2, 4, 8])
def test_every_golden_and_crafted_file_equals_libjpeg(ctxs, library, d):
    from vision_slam_frontend_amd import capi
    files, want = library
    for which, ctx in enumerate(ctxs):
        for name, data in files.items():
            img = want[(name, d)]
            st, got = _decode(ctx, [data], d, img.shape[1], img.shape[0])
            assert st == capi.VSF_OK, (name, d, which, st)
            _check(got[0], img, "%s at 1/%d, decoder %d" % (name, d, which))


def test_mixed_batches_of_one_output_size_per_denominator(ctxs, library):
    """Three calls, one per denominator, each a batch of files whose OUTPUT size is 40 x 30: baseline, progressive and
    restart-interval files of different tables and sampling, of file sizes that differ below the denominator (79 x 59 and
    80 x 60 at 1/2 ...).  The rows' padding is poisoned and must stay poisoned."""
    import PIL.Image as PIL
    import io
    from vision_slam_frontend_amd import capi, synth
    rng = np.random.default_rng(12)
    for d in (2, 4, 8):
        files = []
        for i in range(9):
            W, H = 40 * d - (i % 3) * (d - 1) // 2, 30 * d - (i % 2) * (d - 1)
            assert -(-W // d) == 40 and -(-H // d) == 30
            img = synth.stereo_pair(W, H, 40 + i, n_objects=60)[i & 1]
            kw = dict(quality=int(rng.integers(30, 98)))
            if i % 3 == 1:
                kw["progressive"] = True
            if i % 4 == 2:
                kw["restart_marker_blocks"] = int(rng.integers(1, 9))
            b = io.BytesIO()
            if i % 2:
                rgb = np.stack([img, np.roll(img, 3, 0), 255 - img], 2)
                PIL.fromarray(rgb, "RGB").save(b, "JPEG", subsampling=i % 3, **kw)
            else:
                PIL.fromarray(img, "L").save(b, "JPEG", **kw)
            files.append(b.getvalue())
        st, got = _decode(ctxs[0], files, d, 40, 30, extra=12)
        assert st == capi.VSF_OK
        for i, f in enumerate(files):
            rs, img, warn = ref.imdecode_reduced_gray(f, d, 40, 30)
            assert rs == 0 and warn == 0
            _check(got[i], img, "file %d at 1/%d" % (i, d))


def test_denominator_one_is_the_full_size_call(ctxs, library):
    files, want = library
    ctx = ctxs[0]
    for name in ("ycc420_71x53_q75", "prog_ycc422_71x53_q60", "gray_100x60_restart_rows"):
        img = want[(name, 1)]
        h, w = img.shape
        pitch = (w + 3) // 4 * 4 + 8
        full = torch.full((1, h, pitch), POISON, dtype=torch.uint8, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        ctx.imdecode_gray_batch([files[name]], w, h, full.data_ptr(), h * pitch, pitch)
        ctx.sync()
        st, got = _decode(ctx, [files[name]], 1, w, h)
        assert st == 0 and got.tobytes() == full.cpu().numpy().tobytes(), name
        _check(got[0], img, name)


def test_a_truncated_file_affects_its_own_status_alone(ctxs, library):
    """A file cut inside its entropy-coded data between two good ones: libjpeg reads it WITH a warning, so its pixels are the
    device's own (zero bits, as at full size); the call is accepted, the neighbours are exact, and the next call is clean."""
    from vision_slam_frontend_amd import capi
    files, want = library
    good = files["gray_64x48_noise_q80"]
    cut = good[:len(good) // 2]
    rs, _, warn = ref.imdecode_reduced_gray(cut, 2)
    assert rs == 0 and warn > 0
    st, got = _decode(ctxs[0], [good, cut, good], 2, 32, 24)
    assert st in (capi.VSF_OK, capi.VSF_ERR_INVALID_ARG)   # (vsf_sync's word: a stream that merely ends early is not broken)
    for i in (0, 2):
        _check(got[i], want[("gray_64x48_noise_q80", 2)], "neighbour %d of the truncated file" % i)
    st, got = _decode(ctxs[0], [good], 2, 32, 24)
    assert st == capi.VSF_OK
    _check(got[0], want[("gray_64x48_noise_q80", 2)], "after the truncated file")


def test_refusals_launch_nothing(ctxs, library):
    from vision_slam_frontend_amd import capi
    files, want = library
    good = files["gray_64x48_noise_q80"]
    every = range(1, 6)
    ctx = ctxs[0]
    for d in (0, 3, 16, -2):
        assert _decode(ctx, [good], d, 32, 24, allow_status=every)[0] == capi.VSF_ERR_INVALID_ARG
    assert _decode(ctx, [good], 2, 64, 48, allow_status=every)[0] == capi.VSF_ERR_INVALID_ARG   # the file's own size
    assert _decode(ctx, [good], 4, 32, 24, allow_status=every)[0] == capi.VSF_ERR_INVALID_ARG   # the size of another d
    assert _decode(ctx, [good, files["gray_8x8_q90"]], 2, 32, 24, allow_status=every)[0] == capi.VSF_ERR_INVALID_ARG
    png = sorted((GOLD.parent / "png").glob("*.png"))[0].read_bytes()
    assert _decode(ctx, [good, png], 2, 32, 24, allow_status=every)[0] == capi.VSF_ERR_UNSUPPORTED
    pitch = 40
    dst = torch.full((2, 24, pitch), POISON, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    st = ctx.imdecode_reduced_gray_batch([good, png], 2, 32, 24, dst.data_ptr(), 24 * pitch, pitch, allow_status=every)
    assert st == capi.VSF_ERR_UNSUPPORTED and ctx.sync() == capi.VSF_OK
    assert (dst.cpu().numpy() == POISON).all()   # nothing was launched: not even the good file in front of the PNG
