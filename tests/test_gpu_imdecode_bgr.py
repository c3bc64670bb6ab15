"""vsf_imdecode_bgr_batch -- cv::imdecode(buf, cv::IMREAD_COLOR) for JPEG and PNG payloads on the device -- bit for bit against
the system's libjpeg and libpng driven as OpenCV 3.2 drives them for a three-channel destination (tests/jpeg_ref_bgr.py,
tests/png_ref_bgr.py; tests/test_imdecode_bgr_refs.py pins the two references to Pillow on the CPU and shows that none of the
crafted files below makes them warn).

JPEG: every sampling layout of jpeg_craft.sampling_cases() that libjpeg accepts for a colour read; the sizes at which
jdsample.c's upsamplers change path (component rows of 1, 2 and 3 samples, block and MCU seams, the top and bottom context
rows) with restart intervals of one MCU and of one MCU row; coefficients that drive the conversion out of [0, 255] in every
channel.  Every process jpeg_craft writes: one scan, separate scans, progressive.  PNG: every committed fixture and the streams libpng refuses.  Batches of both formats, pitches wider than
needed with poisoned padding, a refused file in the middle, and files of the library's own encoders read back.  The gray call
on the same files still gives jpeg_ref's bytes."""
import zlib
from pathlib import Path

import numpy as np
import pytest

import imdecode_bgr_cases as cases_bgr
import jpeg_craft as jc
import jpeg_ref
import jpeg_ref_bgr
import png_craft as pc
import png_ref_bgr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = Path(__file__).resolve().parent / "golden"
POISON = 0xEE
GUARD_ROWS = 4
LAYOUTS = cases_bgr.LAYOUTS
upsampler_file = cases_bgr.upsampler_file


@pytest.fixture(scope="module")
def capi():
    from vision_slam_frontend_amd import capi as m
    assert jpeg_ref_bgr.available() and png_ref_bgr.available() and jpeg_ref.available(), "the system's libjpeg / libpng are the references"
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(capi.default_params(640, 480, max_images=2, nfeatures=500))
    yield c
    c.close()


def decode_bgr(capi, ctx, files, w, h, extra_pitch=8, allow_status=(), only=""):
    """One call into a poisoned destination: rows of 3 w bytes rounded up to a dword plus `extra_pitch`, h + 4 rows an image.
    -> (status, status of the sync, (n, h, w, 3)).  Whatever the call answers, only the 3 w bytes of a row may have changed."""
    pitch, rows = (3 * w + 3) // 4 * 4 + extra_pitch, h + GUARD_ROWS
    d = torch.full((len(files), rows, pitch), POISON, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    st = ctx.imdecode_bgr_batch(files, w, h, d.data_ptr(), rows * pitch, pitch, allow_status=allow_status, only=only)
    try:
        sync = ctx.sync()
    except capi.VsfError as e:
        sync = e.status
    got = d.cpu().numpy()
    assert (got[:, h:, :] == POISON).all(), "written below the image"
    assert (got[:, :h, 3 * w:] == POISON).all(), "written behind the 3 * width bytes of a row"
    return st, sync, got[:, :h, :3 * w].reshape(len(files), h, w, 3)


def decode_gray(capi, ctx, files, w, h):
    pitch = (w + 3) // 4 * 4
    d = torch.zeros((len(files), h, pitch), dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.imdecode_gray_batch(files, w, h, d.data_ptr(), h * pitch, pitch)
    assert ctx.sync() == capi.VSF_OK
    return d.cpu().numpy()[:, :, :w]


_ref = {}


def jpeg_want(name, data, w, h):
    """libjpeg's colour read of a crafted file, decoded once: (status, pixels).  A crafted file must not make it warn."""
    if name not in _ref:
        st, img, warn = jpeg_ref_bgr.imdecode_bgr(data, w, h)
        assert warn == 0, (name, warn)
        if img is not None:
            img.setflags(write=False)
        _ref[name] = (st, img)
    return _ref[name]


def check_parity(capi, ctx, cases, w, h, label):
    """cases: [(name, bytes)] of one size, all accepted by libjpeg: one colour call and one gray call, every file twice."""
    files = [c[1] for c in cases] * 2
    st, sync, got = decode_bgr(capi, ctx, files, w, h)
    assert st == capi.VSF_OK and sync == capi.VSF_OK, (label, st, sync)
    gray = decode_gray(capi, ctx, files, w, h)
    for i in range(len(files)):
        name, data = cases[i % len(cases)]
        ref_st, want = jpeg_want(name, data, w, h)
        assert ref_st == 0, (name, ref_st)
        np.testing.assert_array_equal(got[i], want, err_msg="%s, position %d (%s)" % (name, i, label))
        gst, gwant, gwarn = jpeg_ref.imdecode_gray(data, w, h)
        assert gst == 0 and gwarn == 0
        np.testing.assert_array_equal(gray[i], gwant, err_msg="gray read of %s" % name)


def status_of(capi, ctx, data, w, h):
    st, sync, _ = decode_bgr(capi, ctx, [data], w, h, allow_status=(capi.VSF_ERR_INVALID_ARG, capi.VSF_ERR_UNSUPPORTED))
    assert sync == capi.VSF_OK
    return st


# ---- 1. layouts --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("factors", jc.SAMPLING_INTERLEAVED + jc.SAMPLING_SEPARATE_ONLY + jc.SAMPLING_GRAY, ids=jc.sampling_name)
def test_every_layout(capi, ctx, factors):
    """Every file of the set, in every process.  What libjpeg decodes in colour is decoded to its bytes; what it refuses for a
    colour read although a gray read takes it (a chroma factor that does not divide the luminance's: JERR_FRACT_SAMPLE_NOTIMPL
    when the upsampler is set up) is VSF_ERR_INVALID_ARG."""
    seen = 0
    try:
        for serial in (False, True):
            ctx.debug_jpeg_serial(serial)
            for size in ((75, 61), (96, 96), (25, 9), (1, 1)):
                good = []
                for name, data, w, h, f, process in jc.sampling_cases():
                    if f != factors or (w, h) != size:
                        continue
                    seen += 1
                    ref_st, _ = jpeg_want(name, data, w, h)
                    if ref_st == 0:
                        good.append((name, data))
                    else:
                        assert ref_st == 2, (name, ref_st)
                        assert status_of(capi, ctx, data, w, h) == capi.VSF_ERR_INVALID_ARG, name
                if good:
                    check_parity(capi, ctx, good, *size, "serial %d" % serial)
    finally:
        ctx.debug_jpeg_serial(False)
    assert seen > 0


def test_refused_layouts(capi, ctx):
    """More than ten blocks in an interleaved MCU: libjpeg refuses the file, VSF_ERR_INVALID_ARG.  A luminance component below the
    largest factors: the library's one deviation, VSF_ERR_UNSUPPORTED as in the gray call."""
    for name, data, w, h, factors, process, answer in jc.sampling_refusals():
        want = capi.VSF_ERR_INVALID_ARG if answer == "invalid_arg" else capi.VSF_ERR_UNSUPPORTED
        assert status_of(capi, ctx, data, w, h) == want, name
        if answer == "invalid_arg":
            assert jpeg_ref_bgr.imdecode_bgr(data, w, h)[0] != 0, name


# ---- 2. where the upsamplers change path ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_upsampler_paths(capi, ctx, layout):
    """Widths 1 .. 7 give component rows of 1, 2, 3 and 4 samples (the triangle filters are used from 3 on), 16, 17 and 33 cross a
    block and an MCU; heights 1, 2, 8, 9, 16, 17, 33 the top and bottom rows and the context rows across MCU rows."""
    every = cases_bgr.upsampler_cases(layout)
    assert len(every) == len(cases_bgr.WIDTHS) * len(cases_bgr.HEIGHTS)
    for (w, h), cases in every.items():
        check_parity(capi, ctx, cases, w, h, layout)


# ---- 3. range limiting ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["444", "420"])
def test_conversion_leaves_the_range_in_every_channel(capi, ctx, layout):
    """DC coefficients at both ends of what 8-bit samples can be, in every combination over the blocks (Y, Cb and Cr at 0 or 255
    together), a little AC on top: R = Y + 1.402 Cr', G and B likewise leave [0, 255] on both sides."""
    name, data, w, h = cases_bgr.range_case(layout)
    st, want = jpeg_want(name, data, w, h)
    assert st == 0
    for ch in range(3):   # the reference itself reaches both ends in every channel
        assert want[..., ch].min() == 0 and want[..., ch].max() == 255
    check_parity(capi, ctx, [(name, data)], w, h, "range")


# ---- 4. PNG ---------------------------------------------------------------------------------------------------------------------

def test_png_fixtures(capi, ctx):
    """Every committed PNG: gray at every depth, gray + alpha, colour at 8 and 16 bits, palettes (one with transparency), Adam7,
    and the gAMA / sRGB / cHRM files -- no gamma transform is asked of libpng on this path, so they are their samples."""
    by_size = {}
    for f in sorted((GOLDEN / "png").glob("*.png")):
        data = f.read_bytes()
        st, want, info = png_ref_bgr.imdecode_bgr(data)
        assert st == 0 and png_ref_bgr.warnings() == 0, (f.name, st, png_ref_bgr.last_error(), png_ref_bgr.last_warning())
        by_size.setdefault(want.shape[:2], []).append((f.name, data, want))
    assert sum(len(v) for v in by_size.values()) >= 35
    for (h, w), files in by_size.items():
        for only in ("", "png"):
            st, sync, got = decode_bgr(capi, ctx, [f[1] for f in files], w, h, only=only)
            assert st == capi.VSF_OK and sync == capi.VSF_OK
            for i, (name, _, want) in enumerate(files):
                np.testing.assert_array_equal(got[i], want, err_msg=name)


def test_png_streams_libpng_refuses(capi, ctx):
    """The refusals of the gray call's tests, through the colour call: damaged critical chunks and missing PLTE on the host,
    broken compressed data at the next vsf_sync -- and a colour file with an iCCP chunk, which the gray call refuses and this
    one reads, as libpng does."""
    w, h = 96, 64
    yy, xx = np.mgrid[0:h, 0:w]
    img = ((xx * 5 + yy * 3) & 255).astype(np.uint8)
    good = pc.gray8(img, filters=np.arange(h) % 5)

    def status(f, ww=w, hh=h):
        st, sync, got = decode_bgr(capi, ctx, [f], ww, hh, allow_status=(capi.VSF_ERR_INVALID_ARG, capi.VSF_ERR_UNSUPPORTED))
        return st, sync, got

    st, sync, got = status(good)
    assert (st, sync) == (capi.VSF_OK, capi.VSF_OK) and np.array_equal(got[0], np.dstack([img] * 3))
    assert status(good, w + 1, h)[0] == capi.VSF_ERR_INVALID_ARG
    host = [pc.gray8(img, bad_idat_crc=True), good[:-12], good[:40], b"\x89PNG\r\n\x1a\n",
            pc.gray8(img, extra_before=[pc.chunk(b"ABCD", b"xyz")]), pc.write_png(np.zeros((h, w), np.uint8), w, h, 8, 3)]
    for i, f in enumerate(host):
        assert png_ref_bgr.imdecode_bgr(f, w, h)[0] != 0, i
        assert status(f)[0] == capi.VSF_ERR_INVALID_ARG, i
    s = bytearray(pc.idat_stream(good))
    s[-1] ^= 0xFF
    device = [pc.replace_idat(good, bytes(s))] + [pc.replace_idat(good, pc.idat_stream(good)[:-cut]) for cut in (1, 4, 9)]
    for i, f in enumerate(device):
        assert png_ref_bgr.imdecode_bgr(f, w, h)[0] == 2, i
        st, sync, _ = status(f)
        assert (st, sync) == (capi.VSF_OK, capi.VSF_ERR_INVALID_ARG), i
        assert ctx.sync() == capi.VSF_OK
    rgb = np.dstack([img, img // 2, 255 - img])
    iccp = pc.chunk(b"iCCP", b"x\x00\x00" + zlib.compress(b"not a profile"))
    f = pc.write_png(rgb.reshape(h, -1), w, h, 8, 2, extra_before=[iccp])
    ref_st, want, _ = png_ref_bgr.imdecode_bgr(f, w, h)
    assert ref_st == 0 and np.array_equal(want, rgb[..., ::-1])
    st, sync, got = status(f)
    assert (st, sync) == (capi.VSF_OK, capi.VSF_OK)
    np.testing.assert_array_equal(got[0], want)


# ---- 5. batches -----------------------------------------------------------------------------------------------------------------

def mixed_files(rng, w, h):
    """JPEG and PNG, gray and colour, alternating so that the first seven files start a run each and the last two share one: [(name, bytes, want)]."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = ((xx * 3 + yy * 7) & 255).astype(np.uint8)
    rgb = np.dstack([img, 255 - img, (img * 3) & 255]).astype(np.uint8)
    out = []
    for name, data in (("jpeg_420", upsampler_file(rng, w, h, LAYOUTS["420"], 0)), ("png_rgb", pc.write_png(rgb.reshape(h, -1), w, h, 8, 2)),
                       ("jpeg_gray", jc.write_sampling_file(rng, w, h, ((1, 1),), "base")), ("png_gray", pc.gray8(img)),
                       ("jpeg_prog_gray", jc.write_sampling_file(rng, w, h, ((1, 1),), "prog_sep")),
                       ("png_gray_again", pc.gray8(img)),
                       ("jpeg_prog_420", jc.write_sampling_file(rng, w, h, LAYOUTS["420"], "prog_il")),
                       ("jpeg_multi_422", jc.write_sampling_file(rng, w, h, LAYOUTS["422"], "multi_sep")),
                       ("jpeg_422_rst", upsampler_file(rng, w, h, LAYOUTS["422"], "row"))):
        if name.startswith("png"):
            st, want, _ = png_ref_bgr.imdecode_bgr(data, w, h)
            assert st == 0 and png_ref_bgr.warnings() == 0, name
        else:
            st, want = jpeg_want("mixed_%s_%dx%d" % (name, w, h), data, w, h)
            assert st == 0, name
        out.append((name, data, want))
    return out


@pytest.mark.parametrize("extra_pitch", [0, 4, 260])
def test_mixed_batch_and_wide_pitches(capi, ctx, extra_pitch):
    w, h = 45, 19
    files = mixed_files(np.random.default_rng(11), w, h)
    st, sync, got = decode_bgr(capi, ctx, [f[1] for f in files], w, h, extra_pitch=extra_pitch)
    assert st == capi.VSF_OK and sync == capi.VSF_OK
    for i, (name, _, want) in enumerate(files):
        np.testing.assert_array_equal(got[i], want, err_msg=name)


def test_arguments_are_checked(capi, ctx):
    w, h = 45, 19
    f = mixed_files(np.random.default_rng(11), w, h)[1][1]
    need = (3 * w + 3) // 4 * 4
    d = torch.zeros(4 * h * (need + 8), dtype=torch.uint8, device="cuda")
    bad = (capi.VSF_ERR_INVALID_ARG,)
    assert ctx.imdecode_bgr_batch([f], w, h, d.data_ptr(), h * need, need) == capi.VSF_OK and ctx.sync() == capi.VSF_OK
    assert ctx.imdecode_bgr_batch([f], w, h, d.data_ptr(), h * need, need - 4, allow_status=bad) == capi.VSF_ERR_INVALID_ARG
    assert ctx.imdecode_bgr_batch([f], w, h, d.data_ptr(), h * need + 2, need, allow_status=bad) == capi.VSF_ERR_INVALID_ARG
    assert ctx.imdecode_bgr_batch([f], w, h, d.data_ptr() + 2, h * need, need, allow_status=bad) == capi.VSF_ERR_INVALID_ARG
    assert ctx.imdecode_bgr_batch([f], w, h, d.data_ptr(), h * need - 4, need, allow_status=bad) == capi.VSF_ERR_INVALID_ARG
    assert ctx.imdecode_bgr_batch([b"BM" + bytes(60)], w, h, d.data_ptr(), h * need, need,
                                  allow_status=(capi.VSF_ERR_UNSUPPORTED,)) == capi.VSF_ERR_UNSUPPORTED
    assert ctx.sync() == capi.VSF_OK


def test_refused_file_in_the_middle(capi, ctx):
    """As the gray call documents: the runs in front of the refused one have been launched and are not undone, the refused run
    and the runs behind it write nothing."""
    w, h = 45, 19
    files = mixed_files(np.random.default_rng(11), w, h)
    other_size = upsampler_file(np.random.default_rng(3), w + 1, h, LAYOUTS["420"], 0)
    order = [files[0], files[1], ("refused", other_size, None), files[3]]   # four runs: JPEG, PNG, the refused JPEG, PNG
    st, sync, got = decode_bgr(capi, ctx, [f[1] for f in order], w, h, allow_status=(capi.VSF_ERR_INVALID_ARG,))
    assert st == capi.VSF_ERR_INVALID_ARG and sync == capi.VSF_OK
    np.testing.assert_array_equal(got[0], order[0][2])
    np.testing.assert_array_equal(got[1], order[1][2])
    assert (got[2:] == POISON).all()


# ---- 6. round trip --------------------------------------------------------------------------------------------------------------

def _colour_images(w, h):
    rng = np.random.default_rng(w * h)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.dstack([(xx * 4) & 255, (yy * 5) & 255, ((xx + yy) * 3) & 255]).astype(np.uint8)
    return [smooth, rng.integers(0, 256, (h, w, 3)).astype(np.uint8)]


@pytest.mark.parametrize("w,h", [(33, 31), (64, 48), (7, 5)])
def test_own_jpeg_encoder_read_back(capi, ctx, w, h):
    """Three-channel files of vsf_jpeg_encode (the kernels of vsf_jpeg_encode_batch_dev) decode to what libjpeg makes of them."""
    images = _colour_images(w, h)
    with capi.Context(capi.default_params(max(w, 64), max(h, 64), max_images=2, nfeatures=100)) as enc:
        jpegs = enc.jpeg_encode(images, 90) + enc.jpeg_encode(images, 100)
    st, sync, got = decode_bgr(capi, ctx, jpegs, w, h)
    assert st == capi.VSF_OK and sync == capi.VSF_OK
    for i, f in enumerate(jpegs):
        ref_st, want, warn = jpeg_ref_bgr.imdecode_bgr(f, w, h)
        assert ref_st == 0 and warn == 0
        np.testing.assert_array_equal(got[i], want, err_msg="JPEG %d" % i)


@pytest.mark.parametrize("w,h", [(96, 64), (75, 80)])
def test_own_png_encoder_read_back(capi, ctx, w, h):
    """Three-channel files of vsf_png_encode decode to the pixels that went in.  (More than 16384 bytes of scanlines: like libpng
    the encoder declares the smallest zlib window that holds them, and the decoder takes files that declare the full 32 KiB.)"""
    assert 3 * w * h + h > 16384
    images = _colour_images(w, h)
    with capi.Context(capi.default_params(max(w, 64), max(h, 64), max_images=2, nfeatures=100)) as enc:
        pngs = enc.png_encode(images)
    st, sync, got = decode_bgr(capi, ctx, pngs, w, h)
    assert st == capi.VSF_OK and sync == capi.VSF_OK
    for i, f in enumerate(pngs):
        ref_st, want, _ = png_ref_bgr.imdecode_bgr(f, w, h)
        assert ref_st == 0 and png_ref_bgr.warnings() == 0
        np.testing.assert_array_equal(want, images[i])
        np.testing.assert_array_equal(got[i], images[i], err_msg="PNG %d" % i)


def test_committed_jpeg_fixtures(capi, ctx):
    """tests/golden/jpeg and tests/golden/jpeg_enc: one and three components, one scan and progressive."""
    n = 0
    for f in sorted((GOLDEN / "jpeg").glob("*.jpg")) + sorted((GOLDEN / "jpeg_enc").glob("*.jpg")):
        data = f.read_bytes()
        ref_st, want, warn = jpeg_ref_bgr.imdecode_bgr(data)
        assert ref_st == 0 and warn == 0, f.name
        h, w = want.shape[:2]
        st, sync, got = decode_bgr(capi, ctx, [data], w, h, only="jpeg")
        assert st == capi.VSF_OK and sync == capi.VSF_OK, f.name
        np.testing.assert_array_equal(got[0], want, err_msg=f.name)
        n += 1
    assert n >= 37
