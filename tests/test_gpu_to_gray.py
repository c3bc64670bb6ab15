"""vsf_to_gray_batch_dev (csrc/k_ingest.hip: the Bayer kernel in its four orders, the packed-colour kernel, the MONO8 copy)
against tests/pixfmt_ref.py, byte for byte: the sizes at which the kernels change path (a side below 3, one lane, one wave,
256 k + 1 columns whose last source column lies in another wave, more than one strip of rows), noise / all 255 / one
channel at 255, batches of 1 and 5, poisoned source padding, and destination bytes the header does not let the call write."""
import numpy as np
import pytest

import pixfmt_ref as pr

pytestmark = pytest.mark.gpu

BAYER_SIZES = [(3, 3), (4, 3), (5, 4), (255, 17), (256, 16), (257, 33), (260, 18), (513, 5), (2, 2), (2, 5)]
COLOUR_SIZES = [(1, 1), (2, 3), (3, 2), (5, 4), (15, 2), (16, 3), (17, 5), (67, 41), (257, 3)]
POISON_SRC, POISON_DST = 0xA7, 0xC3


@pytest.fixture(scope="module")
def ctx():
    from vision_slam_frontend_amd import capi
    with capi.Context(capi.default_params(64, 64, max_images=2, nfeatures=100), device=0) as c:
        yield c


def _images(pixfmt, w, h, n, content, rng):
    bpp = pr.BPP[pixfmt]
    shape = (n, h, w) if pixfmt not in pr.COLOUR else (n, h, w, bpp)
    if content == "noise":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if content == "all255":
        return np.full(shape, 255, np.uint8)
    ch = int(content[-1])  # one channel (colour) / one site class (Bayer: red, green, blue sites of THIS order) at 255
    if pixfmt in pr.COLOUR:
        img = np.zeros(shape, np.uint8)
        img[..., ch] = 255
        return img
    v = [0, 0, 0]
    v[ch] = 255
    return np.stack([pr.site_constant_mosaic(w, h, pixfmt, *v)] * n)


def _run(ctx, pixfmt, imgs, src_pad, dst_pad, guard_rows=2):
    """Images at a padded source pitch (padding poisoned), result rows at a padded destination pitch inside a poisoned
    buffer with guard rows in front and behind.  Returns (gray images, the whole destination buffer, its geometry)."""
    import torch
    from vision_slam_frontend_amd import capi
    n, h, w = imgs.shape[:3]
    bpp = pr.BPP[pixfmt]
    row = w * bpp
    sp = ((row + 3) & ~3) + 4 * src_pad
    dp = ((w + 3) & ~3) + 4 * dst_pad
    simg, dimg = sp * h + 8 * src_pad, dp * h + 8 * dst_pad
    src = np.full((n, simg), POISON_SRC, np.uint8)
    rows = src[:, :sp * h].reshape(n, h, sp)
    rows[:, :, :row] = imgs.reshape(n, h, row)
    guard = guard_rows * dp
    dst = np.full(guard + n * dimg + guard, POISON_DST, np.uint8)
    d_src = torch.from_numpy(src).to("cuda:0")
    d_dst = torch.from_numpy(dst).to("cuda:0")
    torch.cuda.synchronize()
    st = ctx.to_gray_batch_dev(d_src.data_ptr(), n, w, h, pixfmt, simg, sp, d_dst.data_ptr() + guard, dimg, dp)
    assert st == capi.VSF_OK, st
    assert ctx.sync() == capi.VSF_OK
    got = d_dst.cpu().numpy()
    body = got[guard:guard + n * dimg].reshape(n, dimg)
    return body[:, :dp * h].reshape(n, h, dp)[:, :, :w], got, (guard, dimg, dp)


def _check_untouched(got, geom, n, w, h):
    guard, dimg, dp = geom
    may = np.zeros(got.shape, bool)  # what the header lets the call write: bytes [0, (w + 3) & ~3) of every row
    for i in range(n):
        rows = may[guard + i * dimg:guard + i * dimg + dp * h].reshape(h, dp)
        rows[:, :(w + 3) & ~3] = True
    assert (got[~may] == POISON_DST).all(), "bytes outside the rows' first (w + 3) & ~3 were written"


def _cases(sizes, fmts):
    out = []
    for f in fmts:
        for w, h in sizes:
            out.append(pytest.param(f, w, h, id="fmt%d-%dx%d" % (f, w, h)))
    return out


@pytest.mark.parametrize("pixfmt,w,h", _cases(BAYER_SIZES, pr.BAYER) + _cases(COLOUR_SIZES, pr.COLOUR))
def test_to_gray_matches_reference(ctx, oracle, pixfmt, w, h):
    rng = np.random.default_rng(pixfmt * 100003 + w * 101 + h)
    for n in (1, 5):
        for content in ("noise", "all255", "one0", "one1", "one2"):
            imgs = _images(pixfmt, w, h, n, content, rng)
            want = np.stack([pr.to_gray(im, pixfmt) for im in imgs])
            pad = 0 if (content == "all255" and n == 1) else 1 + (n & 1)  # (once with no padding at all: pitch = the row)
            got, whole, geom = _run(ctx, pixfmt, imgs, pad, pad)
            np.testing.assert_array_equal(got, want, err_msg="%s n=%d" % (content, n))
            _check_untouched(whole, geom, n, w, h)
            if pixfmt in pr.COLOUR:  # columns >= w of a row's last dword: zero
                g, dimg, dp = geom
                tail = whole[g:g + n * dimg].reshape(n, dimg)[:, :dp * h].reshape(n, h, dp)[:, :, w:(w + 3) & ~3]
                assert not tail.any()
            if w < 3 or h < 3:
                assert pixfmt in pr.COLOUR or not got.any()


@pytest.mark.parametrize("pixfmt", list(pr.BAYER) + list(pr.COLOUR))
def test_source_padding_has_no_influence(ctx, oracle, pixfmt):
    # the same images behind two different poisons give the same bytes
    global POISON_SRC
    rng = np.random.default_rng(pixfmt)
    w, h = (257, 33) if pixfmt in pr.BAYER else (67, 41)
    imgs = _images(pixfmt, w, h, 5, "noise", rng)
    keep = POISON_SRC
    try:
        a = _run(ctx, pixfmt, imgs, 2, 1)[0].copy()
        POISON_SRC = 0x00
        b = _run(ctx, pixfmt, imgs, 2, 1)[0].copy()
        POISON_SRC = 0xFF
        c = _run(ctx, pixfmt, imgs, 3, 1)[0].copy()
    finally:
        POISON_SRC = keep
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)


def test_mono8_is_a_copy(ctx, oracle):
    rng = np.random.default_rng(1)
    for w, h in [(1, 1), (5, 4), (67, 41), (257, 3)]:
        imgs = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        got, whole, geom = _run(ctx, pr.PIX_MONO8, imgs, 1, 1)
        np.testing.assert_array_equal(got, imgs)
        _check_untouched(whole, geom, 3, w, h)


def test_rggb_is_the_old_call(ctx, oracle):
    import torch
    from vision_slam_frontend_amd import capi
    m = np.random.default_rng(3).integers(0, 256, (2, 33, 260), dtype=np.uint8)
    d = torch.from_numpy(m).to("cuda:0")
    a = torch.zeros_like(d)
    torch.cuda.synchronize()
    ctx.bayer_bg_to_gray_batch_dev(d.data_ptr(), 2, 260, 33, 260 * 33, 260, a.data_ptr(), 260 * 33, 260)
    assert ctx.sync() == capi.VSF_OK
    got, _, _ = _run(ctx, pr.PIX_BAYER_RGGB8, m, 0, 0)
    np.testing.assert_array_equal(a.cpu().numpy(), got)
    np.testing.assert_array_equal(got, np.stack([oracle.bayer_bg_to_gray(x) for x in m]))


def test_refusals_launch_nothing(ctx):
    import torch
    from vision_slam_frontend_amd import capi
    src = torch.full((4096,), 9, dtype=torch.uint8, device="cuda:0")
    dst = torch.full((4096,), POISON_DST, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    s, d = src.data_ptr(), dst.data_ptr()
    bad = [
        dict(pixfmt=2), dict(pixfmt=15), dict(pixfmt=23), dict(pixfmt=-1),
        dict(pixfmt=pr.PIX_BGR8, sp=44),      # a row is 48 bytes
        dict(pixfmt=pr.PIX_BGRA8, sp=60),
        dict(pixfmt=pr.PIX_BGR8, sp=50),      # not a multiple of 4
        dict(pixfmt=pr.PIX_BGR8, dp=12),      # below (w + 3) & ~3
        dict(pixfmt=pr.PIX_BGR8, s=s + 1), dict(pixfmt=pr.PIX_BGR8, d=d + 2),
        dict(pixfmt=pr.PIX_BGR8, simg=64 * 3), dict(pixfmt=pr.PIX_BGR8, dimg=16 * 3),
        dict(pixfmt=pr.PIX_BGR8, w=0), dict(pixfmt=pr.PIX_BGR8, h=0), dict(pixfmt=pr.PIX_BGR8, n=0),
        dict(pixfmt=pr.PIX_BAYER_GRBG8, w=16385, sp=16388, dp=16388, simg=16388 * 4, dimg=16388 * 4),
        dict(pixfmt=pr.PIX_BGR8, s=0), dict(pixfmt=pr.PIX_BGR8, d=0),
    ]
    for kw in bad:
        a = dict(s=s, n=1, w=16, h=4, pixfmt=0, simg=64 * 4, sp=64, d=d, dimg=16 * 4, dp=16)
        a.update(kw)
        st = ctx.to_gray_batch_dev(a["s"], a["n"], a["w"], a["h"], a["pixfmt"], a["simg"], a["sp"], a["d"], a["dimg"], a["dp"])
        assert st == capi.VSF_ERR_INVALID_ARG, kw
    assert ctx.sync() == capi.VSF_OK
    assert (dst.cpu().numpy() == POISON_DST).all()
