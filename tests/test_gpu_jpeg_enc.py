"""vsf_jpeg_encode_batch_dev / vsf_jpeg_encode == cv::imencode(".jpg") of OpenCV 3.2 (the reference's own instance:
src/test/bag_extract.cc:90), FILE for FILE: every byte equals what the system's libjpeg writes when it is driven as
grfmt_jpeg.cpp drives it (tests/jpeg_enc_ref.py), and what that binding wrote when the fixtures of tests/golden/jpeg_enc were made
(tools/make_jpeg_enc_golden.py) -- no tolerance anywhere.  Sizes: one block, one 4:2:0 MCU, padding in both directions; contents:
see jpeg_enc_ref.make_input (tests/test_jpeg_enc_host.py checks on the CPU that each holds the feature it is named for)."""
import numpy as np
import pytest

import jpeg_enc_ref as ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

if not ref.available():  # (the library is part of the image: a machine without it cannot judge the encoder)
    pytest.skip("libjpeg.so.8 cannot be loaded", allow_module_level=True)

GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    from vision_slam_frontend_amd import capi
    c = capi.Context(capi.default_params(320, 240, max_images=2, nfeatures=100))  # (the encoder ignores this geometry)
    yield c
    c.close()


def _encode_dev(ctx, images, quality, out_stride=None, row_pad=0, poison=0xAB, allow_capacity=False):
    """-> (files or None where the count is -1, counts, the whole output buffer incl. GUARD bytes behind the last slot, status)"""
    from vision_slam_frontend_amd import capi
    dev = torch.device("cuda", 0)
    n = len(images)
    h, w = images[0].shape[:2]
    ch = 1 if images[0].ndim == 2 else 3
    row = w * ch + row_pad
    src = np.full((n, h, row), poison, np.uint8)
    for i, im in enumerate(images):
        src[i, :, :w * ch] = im.reshape(h, w * ch)
    stride = capi.jpeg_encode_capacity(w, h, ch) if out_stride is None else out_stride
    d_src = torch.from_numpy(src).to(dev)
    d_out = torch.full((n * stride + GUARD,), 0xCD, dtype=torch.uint8, device=dev)
    d_n = torch.full((n,), 12345, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.jpeg_encode_batch_dev(d_src.data_ptr(), n, w, h, ch, h * row, row, quality, d_out.data_ptr(), stride, d_n.data_ptr())
    st = ctx.sync(allow_capacity=allow_capacity)
    out, counts = d_out.cpu().numpy(), d_n.cpu().numpy()
    files = [out[i * stride:i * stride + counts[i]].tobytes() if counts[i] >= 0 else None for i in range(n)]
    return files, counts, out, st


@pytest.fixture(scope="module")
def reference_files():
    """Every (content, size, channels, quality) of the matrix, encoded once by libjpeg."""
    want = {}
    for ch, contents in ((1, ref.CONTENTS_GRAY), (3, ref.CONTENTS_BGR)):
        for (w, h) in ref.SIZES:
            for c in contents:
                img = ref.make_input(c, w, h, ch)
                for q in ref.QUALITIES:
                    want[(c, w, h, ch, q)] = ref.imencode(img, q)
    return want


@pytest.mark.parametrize("quality", ref.QUALITIES)
@pytest.mark.parametrize("channels", [1, 3])
def test_files_equal_libjpegs(ctx, reference_files, channels, quality):
    contents = ref.CONTENTS_GRAY if channels == 1 else ref.CONTENTS_BGR
    for (w, h) in ref.SIZES:
        images = [ref.make_input(c, w, h, channels) for c in contents]
        files, counts, _, _ = _encode_dev(ctx, images, quality)
        for c, f in zip(contents, files):
            want = reference_files[(c, w, h, channels, quality)]
            assert f == want, "%s %dx%d x%d q%d: %d bytes, libjpeg wrote %d; first difference at %s" % (
                c, w, h, channels, quality, len(f), len(want),
                next((i for i, (a, b) in enumerate(zip(f, want)) if a != b), "the end"))


def test_files_equal_the_committed_goldens(ctx):
    cases = ref.golden_cases()
    assert len(cases) >= 12
    for name, content, w, h, ch, q in cases:
        want = (ref.GOLDEN / (name + ".jpg")).read_bytes()
        files, _, _, _ = _encode_dev(ctx, [ref.make_input(content, w, h, ch)], q)
        assert files[0] == want, name


@pytest.mark.parametrize("channels", [1, 3])
def test_images_of_many_blocks(ctx, channels):
    """More than one round of the per-image kernels: > 256 blocks, > 4096 scan bytes (200 x 136: 425 blocks gray, 702 in 4:2:0);
    quality 0 means 95."""
    images = [ref.make_input("noise", 200, 136, channels, seed=s) for s in range(2)] + [ref.make_input("ramp", 200, 136, channels)]
    for q in (100, 0):
        files, _, _, _ = _encode_dev(ctx, images, q, row_pad=3)
        for i, im in enumerate(images):
            assert files[i] == ref.imencode(im, q or 95), (channels, q, i)


@pytest.mark.parametrize("channels", [1, 3])
def test_mixed_batch_with_poisoned_row_padding(ctx, channels):
    contents = ref.CONTENTS_GRAY if channels == 1 else ref.CONTENTS_BGR
    images = [ref.make_input(contents[i % len(contents)], 33, 31, channels, seed=i) for i in range(32)]
    for i in range(len(contents), 32):  # (the later rounds: the same contents with noise mixed in, so that all 32 differ)
        noise = ref.make_input("noise", 33, 31, channels, seed=i)
        images[i] = np.where(noise > 200, noise, images[i]).astype(np.uint8)
    assert len({im.tobytes() for im in images}) == 32
    want = [ref.imencode(im, 95) for im in images]
    for poison in (0xAB, 0x00):
        files, _, _, _ = _encode_dev(ctx, images, 95, row_pad=13, poison=poison)
        assert files == want


def test_overflow_of_one_slot(ctx):
    from vision_slam_frontend_amd import capi
    images = [ref.make_input(c, 33, 31, 3) for c in ("flat128", "ramp", "noise", "zz63")]
    want = [ref.imencode(im, 100) for im in images]
    big = max(range(4), key=lambda i: len(want[i]))
    assert big == 2 and all(len(want[i]) < len(want[2]) - 1 for i in (0, 1, 3))
    stride = len(want[2]) - 1  # one byte short for the noise image alone
    for order in ([0, 1, 2, 3], [0, 1, 3, 2]):  # ... in the middle of the batch, and as its last slot (the guard behind it)
        files, counts, out, st = _encode_dev(ctx, [images[i] for i in order], 100, out_stride=stride, allow_capacity=True)
        assert st == capi.VSF_ERR_CAPACITY
        for slot, i in enumerate(order):
            if i == 2:
                assert counts[slot] == -1 and files[slot] is None
            else:
                assert files[slot] == want[i], (order, slot)
                # ... and the rest of a neighbour's slot is as it was
                assert (out[slot * stride + counts[slot]:(slot + 1) * stride] == 0xCD).all()
        assert (out[4 * stride:] == 0xCD).all() and len(out) == 4 * stride + GUARD
        assert ctx.sync() == capi.VSF_OK  # (the status is reported once)
    # the exact size fits
    files, counts, out, st = _encode_dev(ctx, [images[2]], 100, out_stride=len(want[2]))
    assert files[0] == want[2] and (out[len(want[2]):] == 0xCD).all()
    # a slot shorter than the header: nothing at all is written
    files, counts, out, st = _encode_dev(ctx, images, 100, out_stride=100, allow_capacity=True)
    assert st == capi.VSF_ERR_CAPACITY and (counts == -1).all() and (out == 0xCD).all()


def test_host_pointer_call_and_argument_checks(ctx):
    from vision_slam_frontend_amd import capi
    images = [ref.make_input(c, 17, 9, 3) for c in ref.CONTENTS_BGR]
    assert ctx.jpeg_encode(images, 50) == [ref.imencode(im, 50) for im in images]
    gray = [ref.make_input("noise", 64, 48, 1)]
    assert ctx.jpeg_encode(gray) == [ref.imencode(gray[0], 95)]
    with pytest.raises(capi.VsfError) as e:
        ctx.jpeg_encode(gray, 100, out_stride=1000)
    assert e.value.status == capi.VSF_ERR_CAPACITY
    L = capi.lib()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    n = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    for w, h, ch, q, row in ((0, 8, 1, 95, 8), (8, 0, 1, 95, 8), (65536, 8, 1, 95, 65536), (8, 8, 2, 95, 16), (8, 8, 4, 95, 32),
                             (8, 8, 1, 101, 8), (8, 8, 1, -1, 8), (8, 8, 3, 95, 23)):
        st = L.vsf_jpeg_encode_batch_dev(ctx._h, d.data_ptr(), 1, w, h, ch, row * max(h, 1), row, q, d.data_ptr(), 2048, n.data_ptr())
        assert st == capi.VSF_ERR_INVALID_ARG, (w, h, ch, q, row)
    assert L.vsf_jpeg_encode_batch_dev(ctx._h, d.data_ptr(), 1, 65535, 65535, 1, 65535 * 65535, 65535, 95, d.data_ptr(), 2048,
                                       n.data_ptr()) == capi.VSF_ERR_UNSUPPORTED
    assert ctx.sync() == capi.VSF_OK


def test_round_trip_through_the_decoder(ctx):
    """vsf_jpeg_decode_gray_batch of the encoder's 1-channel files == libjpeg's decode of the reference's files."""
    import jpeg_ref
    from vision_slam_frontend_amd import capi
    assert jpeg_ref.available()
    w, h = 64, 48
    images = [ref.make_input(c, w, h, 1) for c in ref.CONTENTS_GRAY]
    files, _, _, _ = _encode_dev(ctx, images, 95)
    d = torch.full((len(files), h, w), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.jpeg_decode_gray_batch(files, w, h, d.data_ptr(), h * w, w)
    assert ctx.sync() == capi.VSF_OK
    got = d.cpu().numpy()
    for i, im in enumerate(images):
        st, want, _ = jpeg_ref.imdecode_gray(ref.imencode(im, 95), w, h)
        assert st == 0
        np.testing.assert_array_equal(got[i], want, err_msg=ref.CONTENTS_GRAY[i])
