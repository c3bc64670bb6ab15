"""vsf_bag_extract_batch -- src/test/bag_extract.cc:73-90 as one call -- against the chain of the references, file for file and
byte for byte:
    tests/jpeg_ref_bgr.py / png_ref_bgr.py (cv::imdecode(data, 1))  ->  [..., 0] (cv::split, channel 0)
    ->  tests/bayer_bgr_ref.py (cvtColor(COLOR_Bayer??2BGR))  ->  tests/jpeg_enc_ref.py (cv::imwrite(".jpg"))
on the committed fixtures: one-component baseline and progressive JPEG, 4:4:4 and 4:2:0 colour JPEG on a Bayer topic (the mosaic
is the BLUE channel there, not the gray read), gray and RGB PNG, a 1 x 1 file; with and without the flag, in all four orders, at
qualities 0 (= 95) and 50, JPEG and PNG mixed in one call.  And against the three calls by hand, the capacity rule, and the
refusals."""
from pathlib import Path

import numpy as np
import pytest

import bayer_bgr_ref as br
import jpeg_enc_ref
import jpeg_ref_bgr
import pixfmt_ref as pr
import png_craft as pc
import png_ref_bgr

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
# (size) -> fixtures of that size, what each is here for
GROUPS = {
    "gray_mixed_160x120": (160, 120, ["jpeg/gray_160x120_optimized.jpg", "png/pil_photo_level6.png", "jpeg/prog_gray_160x120_restart5.jpg",
                                      "png/craft_gray16.png", "jpeg/gray_160x120_restart4.jpg", "png/craft_gray_alpha8.png"]),
    "ycc444_40x40": (40, 40, ["jpeg/ycc444_40x40_q90.jpg", "jpeg/prog_ycc444_40x40_q92.jpg"]),
    "ycc420_71x53": (71, 53, ["jpeg/ycc420_71x53_q75.jpg", "jpeg/ycc422_71x53_q75.jpg", "jpeg/prog_ycc422_71x53_q60.jpg"]),
    "png_rgb_96x64": (96, 64, ["png/colour_rgb8.png", "png/adam7_gray8.png", "png/colour_rgba8.png", "png/colour_palette4.png",
                               "png/colour_rgb8_gama45455.png"]),
    "gray_1x1": (1, 1, ["jpeg/gray_1x1_q75.jpg"]),
    "gray_33x17": (33, 17, ["jpeg/gray_33x17_q95.jpg", "jpeg/prog_gray_33x17_q30.jpg"]),
}
_decoded = {}


@pytest.fixture(scope="module")
def capi():
    from vision_slam_frontend_amd import capi as m
    assert jpeg_ref_bgr.available() and png_ref_bgr.available() and jpeg_enc_ref.available(), "the system's libjpeg / libpng are the references"
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(capi.default_params(64, 64, max_images=2, nfeatures=100))
    yield c
    c.close()


def _read(name):
    return (GOLDEN / name).read_bytes()


def _colour_read(name, w, h):
    """cv::imdecode(data, 1) by the reference, once per file."""
    if name not in _decoded:
        ref = jpeg_ref_bgr if name.endswith(".jpg") else png_ref_bgr
        st, img, _ = ref.imdecode_bgr(_read(name), w, h)
        assert st == 0 and img.shape == (h, w, 3), (name, st)
        img.setflags(write=False)
        _decoded[name] = img
    return _decoded[name]


def _want(name, w, h, bayer, quality):
    img = _colour_read(name, w, h)
    if bayer:
        img = br.bayer_to_bgr(img[..., 0], bayer)
    return jpeg_enc_ref.imencode(img, quality if quality else 95)


@pytest.mark.parametrize("group", list(GROUPS))
def test_files_are_the_reference_chain(capi, ctx, group):
    w, h, names = GROUPS[group]
    files = [_read(n) for n in names]
    for bayer in (0,) + pr.BAYER:
        for quality in (0, 50):
            st, got = ctx.bag_extract_batch(files, w, h, bayer, quality)
            assert st == capi.VSF_OK, (bayer, quality, st)
            for name, g in zip(names, got):
                assert g == _want(name, w, h, bayer, quality), "%s bayer %d quality %d" % (name, bayer, quality)


def test_the_mosaic_of_a_colour_file_is_its_blue_channel(capi, ctx):
    """The fixtures must be able to tell: blue, the gray read and the two other channels of the 4:2:0 file differ, and so do the
    files made of them."""
    w, h, names = GROUPS["ycc420_71x53"]
    name = names[0]
    img = _colour_read(name, w, h)
    gray = br.bgr_to_gray(img)
    assert (img[..., 0] != gray).mean() > 0.5 and (img[..., 0] != img[..., 1]).mean() > 0.5
    st, got = ctx.bag_extract_batch([_read(name)], w, h, pr.PIX_BAYER_RGGB8, 0)
    assert st == capi.VSF_OK
    assert got[0] == jpeg_enc_ref.imencode(br.bayer_to_bgr(img[..., 0], pr.PIX_BAYER_RGGB8), 95)
    assert got[0] != jpeg_enc_ref.imencode(br.bayer_to_bgr(gray, pr.PIX_BAYER_RGGB8), 95)


@pytest.mark.parametrize("group", ["gray_mixed_160x120", "ycc420_71x53"])
def test_equals_the_three_calls_by_hand(capi, ctx, group):
    import torch
    w, h, names = GROUPS[group]
    files = [_read(n) for n in names]
    n, bp, mp = len(files), (3 * w + 3) & ~3, (w + 3) & ~3
    cap = int(capi.lib().vsf_jpeg_encode_capacity(w, h, 3))
    for bayer in (0, pr.PIX_BAYER_RGGB8, pr.PIX_BAYER_GBRG8):
        d_bgr = torch.zeros((n, h, bp), dtype=torch.uint8, device="cuda:0")
        d_out = torch.zeros((n, cap), dtype=torch.uint8, device="cuda:0")
        d_n = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.imdecode_bgr_batch(files, w, h, d_bgr.data_ptr(), h * bp, bp)
        assert ctx.sync() == capi.VSF_OK
        d_img = d_bgr
        if bayer:
            d_mosaic = torch.zeros((n, h, mp), dtype=torch.uint8, device="cuda:0")
            d_mosaic[:, :, :w] = d_bgr[:, :, :3 * w:3]  # cv::split -> channel 0
            d_img = torch.zeros((n, h, bp), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            assert ctx.to_bgr_batch_dev(d_mosaic.data_ptr(), n, w, h, bayer, h * mp, mp, d_img.data_ptr(), h * bp, bp) == capi.VSF_OK
        ctx.jpeg_encode_batch_dev(d_img.data_ptr(), n, w, h, 3, h * bp, bp, 50, d_out.data_ptr(), cap, d_n.data_ptr())
        assert ctx.sync() == capi.VSF_OK
        sizes, out = d_n.cpu().numpy(), d_out.cpu().numpy()
        st, got = ctx.bag_extract_batch(files, w, h, bayer, 50)
        assert st == capi.VSF_OK
        for i in range(n):
            assert got[i] == out[i, :sizes[i]].tobytes(), (names[i], bayer)


def test_a_file_that_does_not_fit_is_minus_one_and_the_others_are_intact(capi, ctx):
    w, h, names = GROUPS["gray_mixed_160x120"]
    files = [_read(n) for n in names]
    st, full = ctx.bag_extract_batch(files, w, h, pr.PIX_BAYER_RGGB8, 0)
    assert st == capi.VSF_OK
    sizes = sorted(len(f) for f in full)
    assert sizes[0] < sizes[-1]
    stride = sizes[-1] - 1  # the largest file (or files) does not fit, every smaller one does
    st, got = ctx.bag_extract_batch(files, w, h, pr.PIX_BAYER_RGGB8, 0, out_stride=stride)
    assert st == capi.VSF_ERR_CAPACITY
    for f, g in zip(full, got):
        assert g == (f if len(f) <= stride else None)
    assert any(g is None for g in got) and any(g is not None for g in got)
    st, again = ctx.bag_extract_batch(files, w, h, pr.PIX_BAYER_RGGB8, 0)  # (nothing of the refusal stays behind)
    assert st == capi.VSF_OK and again == full


def test_damaged_files_and_other_sizes_give_the_decoders_status_and_nothing(capi, ctx):
    import torch
    w, h, names = GROUPS["gray_mixed_160x120"]
    files = [_read(n) for n in names]
    refusals = (capi.VSF_ERR_INVALID_ARG, capi.VSF_ERR_UNSUPPORTED)
    yy, xx = np.mgrid[0:h, 0:w]
    good = pc.gray8(((xx * 5 + yy * 3) & 255).astype(np.uint8))
    broken = pc.replace_idat(good, pc.idat_stream(good)[:-4])  # headers and chunks intact: the DEVICE finds the stream cut short
    assert png_ref_bgr.imdecode_bgr(good, w, h)[0] == 0 and png_ref_bgr.imdecode_bgr(broken, w, h)[0] == 2
    cases = {
        "cut inside the headers": files[0][:100],
        "another size": _read("jpeg/gray_33x17_q95.jpg"),
        "a png of another size": _read("png/colour_rgb8.png"),
        "compressed data libpng refuses": broken,
    }
    d = torch.zeros((len(files), h, 3 * w), dtype=torch.uint8, device="cuda:0")
    for label, bad in cases.items():
        batch = files[:2] + [bad] + files[2:4]
        # what the colour decoder says to the same list, in the call or at the sync
        want = ctx.imdecode_bgr_batch(batch, w, h, d.data_ptr(), h * 3 * w, 3 * w, allow_status=refusals)
        try:
            synced = ctx.sync()
        except capi.VsfError as e:
            synced = e.status
        want = want if want != capi.VSF_OK else synced
        assert want in refusals, (label, want)
        for bayer in (0, pr.PIX_BAYER_RGGB8):
            st, got = ctx.bag_extract_batch(batch, w, h, bayer, 0, allow_status=refusals)
            assert st == want, (label, st, want)
            assert got == [None] * len(batch), label
    st, got = ctx.bag_extract_batch(files, w, h, pr.PIX_BAYER_RGGB8, 0)  # the context goes on
    assert st == capi.VSF_OK and got[0] == _want(names[0], w, h, pr.PIX_BAYER_RGGB8, 0)


def test_arguments_are_checked(capi, ctx):
    w, h, names = GROUPS["gray_33x17"]
    files = [_read(n) for n in names]
    for code in (pr.PIX_BGR8, pr.PIX_RGB8, pr.PIX_BGRA8, pr.PIX_RGBA8, 2, 15, 23, -1):  # (0 = MONO8's code means "no mosaic")
        st, got = ctx.bag_extract_batch(files, w, h, code, 0, allow_status=(capi.VSF_ERR_INVALID_ARG,))
        assert st == capi.VSF_ERR_INVALID_ARG and got == [None, None], code
    for kw in (dict(quality=-1), dict(quality=101), dict(out_stride=0)):
        st, got = ctx.bag_extract_batch(files, w, h, 0, **{"quality": 0, **kw}, allow_status=(capi.VSF_ERR_INVALID_ARG,))
        assert st == capi.VSF_ERR_INVALID_ARG and got == [None, None], kw
    st, got = ctx.bag_extract_batch([b"BM" + bytes(64)], w, h, 0, 0, allow_status=(capi.VSF_ERR_UNSUPPORTED,))
    assert st == capi.VSF_ERR_UNSUPPORTED and got == [None]
    assert ctx.sync() == capi.VSF_OK
