"""vsf_png_encode_batch_dev / vsf_png_encode (k_png_enc.hip) against the system's libpng driven as cv::imencode(".png") of
OpenCV 3.2 drives it (tests/png_enc_ref.py): the FILES are equal byte for byte -- and equal to the committed files of
tests/golden/png_enc, so that the test still bites where the library differs."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import png_enc_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

if not ref.available():
    pytest.skip("libpng16.so.16 cannot be loaded", allow_module_level=True)


@pytest.fixture(scope="module")
def ctx():
    from vision_slam_frontend_amd import capi
    c = capi.Context(capi.default_params(320, 240, max_images=2, nfeatures=100))  # (the encoder ignores this geometry)
    yield c
    c.close()


def _dev(ctx, imgs, pad=0, out_stride=None, tail=64):
    """Encodes equally sized images through vsf_png_encode_batch_dev -> (files, byte counts, the bytes behind every slot)."""
    import torch
    from vision_slam_frontend_amd import capi
    imgs = np.stack(imgs)
    n, h, w = imgs.shape[:3]
    ch = 1 if imgs.ndim == 3 else 3
    row = w * ch + pad
    src = np.full((n, h, row), 0xA5, np.uint8)  # poisoned row padding
    src[:, :, :w * ch] = imgs.reshape(n, h, w * ch)
    stride = capi.png_encode_capacity(w, h, ch) if out_stride is None else out_stride
    d_src = torch.from_numpy(src).cuda()
    # without out_stride: slots of the capacity plus `tail` spare bytes each; with it: slots of exactly out_stride bytes (they are
    # out_stride apart by definition) and `tail` guard bytes behind the last one
    slot = stride + tail if out_stride is None else stride
    d_out = torch.full((n * slot + tail,), 0x5A, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx.png_encode_batch_dev(d_src.data_ptr(), n, w, h, ch, h * row, row, d_out.data_ptr(), slot, d_n.data_ptr())
    if out_stride is None:  # (a short slot leaves VSF_ERR_CAPACITY for the caller's vsf_sync)
        ctx.sync()
    else:
        torch.cuda.synchronize()
    flat = d_out.cpu().numpy()
    return flat[:n * slot].reshape(n, slot), d_n.cpu().numpy(), flat[n * slot:]


def _check_dev(ctx, imgs, pad=0):
    from vision_slam_frontend_amd import capi
    out, nb, guard = _dev(ctx, imgs, pad)
    assert (guard == 0x5A).all()
    ch = 1 if imgs[0].ndim == 2 else 3
    cap = capi.png_encode_capacity(imgs[0].shape[1], imgs[0].shape[0], ch)
    for i, img in enumerate(imgs):
        want = ref.imencode(img)
        assert nb[i] == len(want), (i, nb[i], len(want))
        assert out[i, :nb[i]].tobytes() == want, i
        assert (out[i, nb[i]:] == 0x5A).all()  # the bytes behind the file and behind the slot stay untouched


CONTENTS = ["flat0", "flat200", "noise", "few2", "few3", "few4", "ramp"]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", ref.SIZES, ids=lambda s: "%dx%d" % s)
def test_files_equal_libpngs(ctx, size, channels):
    w, h = size
    imgs = [ref.make_input(c, w, h, channels) for c in CONTENTS]
    _check_dev(ctx, imgs, pad=5)                                  # a batch of distinct images, poisoned row padding
    got = ctx.png_encode(imgs)                                    # the host-pointer call
    assert got == [ref.imencode(i) for i in imgs]


def test_stereo_canvas_1280x480_bgr(ctx):
    imgs = [ref.make_input("few4", 1280, 480, 3), ref.make_input("channels", 1280, 480, 3)]
    _check_dev(ctx, imgs)


def test_run_lengths_and_filter_byte(ctx):
    _check_dev(ctx, [ref.make_input("runs", 2200, 3, 1)])
    _check_dev(ctx, [ref.make_input("filterbyte", 64, 48, 1)])
    _check_dev(ctx, [ref.make_input("channels", 33, 31, 3)], pad=3)


@pytest.mark.parametrize("symbols", [16382, 16383, 16384, 16385])
def test_block_boundaries(ctx, symbols):
    img = ref.with_symbols(symbols)
    blocks = ref.deflate_blocks(ref.idat(ref.imencode(img)))
    assert ref.count_symbols(ref.filtered(img)) == symbols and len(blocks) == symbols // 16383 + 1
    _check_dev(ctx, [img])


@pytest.mark.parametrize("residue", [8191, 8192, 8193])
def test_idat_chunk_boundaries(ctx, residue):
    img = ref.with_stream_length(residue)
    assert len(ref.idat(ref.imencode(img))) % 8192 == residue % 8192
    _check_dev(ctx, [img])


def test_goldens(ctx):
    cases = ref.golden_cases()
    assert len(cases) >= 10
    for name, content, w, h, ch in cases:
        got = ctx.png_encode([ref.make_input(content, w, h, ch)])[0]
        assert got == (ref.GOLDEN / (name + ".png")).read_bytes(), name


def test_slot_one_byte_short(ctx):
    """The middle file's slot is one byte short: it reports -1 and VSF_ERR_CAPACITY, its neighbours are delivered, and nothing is
    written behind any slot."""
    import ctypes as C
    from vision_slam_frontend_amd import capi
    imgs = [ref.make_input("flat3", 33, 31, 1), ref.make_input("noise", 33, 31, 1), ref.make_input("ramp", 33, 31, 1)]
    want = [ref.imencode(i) for i in imgs]
    assert len(want[1]) > len(want[0]) and len(want[1]) > len(want[2])
    stride = len(want[1]) - 1
    src = np.stack(imgs)
    out = np.full((3, stride), 0x5A, np.uint8)
    nb = np.zeros(3, np.int32)
    st = capi.lib().vsf_png_encode(ctx._h, src.ctypes.data_as(C.c_void_p), 3, 33, 31, 1, 33 * 31, 33,
                                   out.ctypes.data_as(C.c_void_p), stride, nb.ctypes.data_as(C.c_void_p))
    assert st == capi.VSF_ERR_CAPACITY
    assert nb.tolist() == [len(want[0]), -1, len(want[2])]
    assert out[0, :nb[0]].tobytes() == want[0] and out[2, :nb[2]].tobytes() == want[2]
    assert (out[0, nb[0]:] == 0x5A).all() and (out[1] == 0x5A).all() and (out[2, nb[2]:] == 0x5A).all()
    # the device form: the same, and the bytes behind every slot stay untouched
    o, n, guard = _dev(ctx, imgs, out_stride=stride, tail=64)  # (64 guard bytes behind the last slot)
    assert n.tolist() == [len(want[0]), -1, len(want[2])]
    assert o[0, :n[0]].tobytes() == want[0] and o[2, :n[2]].tobytes() == want[2] and (o[1] == 0x5A).all()
    assert (o[0, n[0]:] == 0x5A).all() and (o[2, n[2]:] == 0x5A).all() and (guard == 0x5A).all()
    # ... and with the SHORT slot last, so that an overrun would land in the guard
    o, n, guard = _dev(ctx, [imgs[0], imgs[2], imgs[1]], out_stride=stride, tail=64)
    assert n.tolist() == [len(want[0]), len(want[2]), -1] and (o[2] == 0x5A).all() and (guard == 0x5A).all()
    assert capi.lib().vsf_sync(ctx._h) == capi.VSF_ERR_CAPACITY
    assert capi.lib().vsf_sync(ctx._h) == capi.VSF_OK
    # exactly the file's size is enough
    assert ctx.png_encode([imgs[1]], out_stride=len(want[1])) == [want[1]]


def test_round_trip(ctx):
    """The real libpng and the device's own PNG decoder read the gray files back to the input.  160 x 120: more than 16384
    filtered bytes, so the zlib header declares the full window, the only one the device decoder accepts."""
    import png_ref
    import torch
    from vision_slam_frontend_amd import capi
    assert png_ref.available()
    w, h = 160, 120
    imgs = [ref.make_input(c, w, h, 1) for c in ("noise", "few3", "ramp", "flat9")]
    files = ctx.png_encode(imgs)
    for img, f in zip(imgs, files):
        assert f[41:43] == b"\x78\x01"
        st, back, info = png_ref.imdecode_gray(f, w, h)
        assert st == 0 and info[:3] == (8, 0, 0) and np.array_equal(back, img)
    for sw, sh in ref.SIZES:  # the real libpng reads every size back, the small ones with their shrunken window included
        if sw * sh > 70000:
            continue
        small = [ref.make_input(c, sw, sh, 1) for c in ("noise", "few3", "flat9")]
        for img, f in zip(small, ctx.png_encode(small)):
            st, back, info = png_ref.imdecode_gray(f, sw, sh)
            assert st == 0 and np.array_equal(back, img), (sw, sh)
    with capi.Context(capi.default_params(w, h, max_images=4, nfeatures=100)) as c:  # (the decoder reads at the context's size)
        d = torch.zeros((len(files), h, w), dtype=torch.uint8, device="cuda")
        c.png_decode_gray_batch(files, w, h, d.data_ptr(), h * w, w)
        c.sync()
        assert np.array_equal(d.cpu().numpy(), np.stack(imgs))
