"""vsf_to_bgr_batch_dev / vsf_to_bgr (csrc/k_to_bgr.hip: the Bayer kernel in its four orders, the packed kernel in its five
conversions) against tests/bayer_bgr_ref.py, byte for byte: the sizes at which the kernels change path (a side below 3, one lane,
one wave, 256 k + 1 columns whose last source column lies in another wave, more than one strip of rows, rows whose 3 w bytes
end inside a dword), noise / all 255 / one channel or site class at 255, batches of 1 and 5, poisoned source padding, and
destination bytes the header does not let the call write.  And the property that ties it to the gray call:
to_gray(to_bgr(x), BGR8) == to_gray(x) through the existing kernels, for every format."""
import numpy as np
import pytest

import bayer_bgr_ref as br
import pixfmt_ref as pr

pytestmark = pytest.mark.gpu

BAYER_SIZES = [(3, 3), (4, 3), (5, 4), (255, 17), (256, 16), (257, 33), (260, 18), (513, 5), (2, 2), (2, 5)]
PACKED_SIZES = [(1, 1), (2, 3), (3, 2), (5, 4), (15, 2), (16, 3), (17, 5), (67, 41), (257, 3)]
PACKED = (pr.PIX_MONO8,) + pr.COLOUR
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
    if pixfmt == pr.PIX_MONO8:  # (no channels: a column in three at 255)
        img = np.zeros(shape, np.uint8)
        img[..., ch::3] = 255
        return img
    v = [0, 0, 0]
    v[ch] = 255
    return np.stack([pr.site_constant_mosaic(w, h, pixfmt, *v)] * n)


def _rows(w):
    return (3 * w + 3) & ~3


def _run(ctx, pixfmt, imgs, src_pad, dst_pad, guard_rows=2, poison_src=POISON_SRC):
    """Images at a padded source pitch (padding poisoned), result rows at a padded destination pitch inside a poisoned
    buffer with guard rows in front and behind.  Returns (B G R images, the whole destination buffer, its geometry)."""
    import torch
    from vision_slam_frontend_amd import capi
    n, h, w = imgs.shape[:3]
    row = w * pr.BPP[pixfmt]
    sp = ((row + 3) & ~3) + 4 * src_pad
    dp = _rows(w) + 4 * dst_pad
    simg, dimg = sp * h + 8 * src_pad, dp * h + 8 * dst_pad
    src = np.full((n, simg), poison_src, np.uint8)
    src[:, :sp * h].reshape(n, h, sp)[:, :, :row] = imgs.reshape(n, h, row)
    guard = guard_rows * dp
    dst = np.full(guard + n * dimg + guard, POISON_DST, np.uint8)
    d_src = torch.from_numpy(src).to("cuda:0")
    d_dst = torch.from_numpy(dst).to("cuda:0")
    torch.cuda.synchronize()
    st = ctx.to_bgr_batch_dev(d_src.data_ptr(), n, w, h, pixfmt, simg, sp, d_dst.data_ptr() + guard, dimg, dp)
    assert st == capi.VSF_OK, st
    assert ctx.sync() == capi.VSF_OK
    got = d_dst.cpu().numpy()
    body = got[guard:guard + n * dimg].reshape(n, dimg)
    return body[:, :dp * h].reshape(n, h, dp)[:, :, :3 * w].reshape(n, h, w, 3), got, (guard, dimg, dp)


def _check_untouched_and_tails(got, geom, n, w, h):
    guard, dimg, dp = geom
    may = np.zeros(got.shape, bool)  # what the header lets the call write: bytes [0, (3 w + 3) & ~3) of every row
    for i in range(n):
        rows = may[guard + i * dimg:guard + i * dimg + dp * h].reshape(h, dp)
        rows[:, :_rows(w)] = True
    assert (got[~may] == POISON_DST).all(), "bytes outside the rows' first (3 w + 3) & ~3 were written"
    tail = got[guard:guard + n * dimg].reshape(n, dimg)[:, :dp * h].reshape(n, h, dp)[:, :, 3 * w:_rows(w)]
    assert not tail.any(), "the bytes behind 3 w - 1 of a row's last dword are not zero"


def _to_gray_dev(ctx, bgr):
    """vsf_to_gray_batch_dev(VSF_PIX_BGR8) -- the existing call -- on (n, h, w, 3) images."""
    import torch
    from vision_slam_frontend_amd import capi
    n, h, w = bgr.shape[:3]
    sp, dp = _rows(w), (w + 3) & ~3
    src = np.zeros((n, h, sp), np.uint8)
    src[:, :, :3 * w] = bgr.reshape(n, h, 3 * w)
    d_src = torch.from_numpy(src).to("cuda:0")
    d_dst = torch.zeros((n, h, dp), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert ctx.to_gray_batch_dev(d_src.data_ptr(), n, w, h, pr.PIX_BGR8, sp * h, sp, d_dst.data_ptr(), dp * h, dp) == capi.VSF_OK
    assert ctx.sync() == capi.VSF_OK
    return d_dst.cpu().numpy()[:, :, :w]


def _cases(sizes, fmts):
    return [pytest.param(f, w, h, id="fmt%d-%dx%d" % (f, w, h)) for f in fmts for w, h in sizes]


@pytest.mark.parametrize("pixfmt,w,h", _cases(BAYER_SIZES, pr.BAYER) + _cases(PACKED_SIZES, PACKED))
def test_to_bgr_matches_reference(ctx, oracle, pixfmt, w, h):
    rng = np.random.default_rng(pixfmt * 100003 + w * 101 + h)
    for n in (1, 5):
        for content in ("noise", "all255", "one0", "one1", "one2"):
            imgs = _images(pixfmt, w, h, n, content, rng)
            want = np.stack([br.to_bgr(im, pixfmt) for im in imgs])
            pad = 0 if (content == "all255" and n == 1) else 1 + (n & 1)  # (once with no padding at all: pitch = the row)
            got, whole, geom = _run(ctx, pixfmt, imgs, pad, pad)
            np.testing.assert_array_equal(got, want, err_msg="%s n=%d" % (content, n))
            _check_untouched_and_tails(whole, geom, n, w, h)
            if pixfmt in pr.BAYER and (w < 3 or h < 3):
                assert not got.any()
            if content == "noise":  # the existing gray kernels agree: gray of the colour image is the gray of the frame
                np.testing.assert_array_equal(_to_gray_dev(ctx, got), np.stack([pr.to_gray(im, pixfmt) for im in imgs]))
                np.testing.assert_array_equal(_to_gray_dev(ctx, got), _to_gray_of(ctx, pixfmt, imgs))


def _to_gray_of(ctx, pixfmt, imgs):
    """vsf_to_gray (host to host, the existing call) of the raw frames."""
    return ctx.to_gray(imgs, pixfmt)


@pytest.mark.parametrize("pixfmt", list(pr.BAYER) + list(PACKED))
def test_source_padding_has_no_influence(ctx, oracle, pixfmt):
    # the same images behind three different poisons give the same bytes
    rng = np.random.default_rng(pixfmt)
    w, h = (257, 33) if pixfmt in pr.BAYER else (67, 41)
    imgs = _images(pixfmt, w, h, 5, "noise", rng)
    a = _run(ctx, pixfmt, imgs, 2, 1)[0].copy()
    b = _run(ctx, pixfmt, imgs, 2, 1, poison_src=0x00)[0].copy()
    c = _run(ctx, pixfmt, imgs, 3, 1, poison_src=0xFF)[0].copy()
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)


@pytest.mark.parametrize("pixfmt", list(pr.BAYER) + list(PACKED))
def test_host_to_host_at_odd_addresses_and_pitches(ctx, oracle, pixfmt):
    from vision_slam_frontend_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(pixfmt + 77)
    w, h = (261, 19) if pixfmt in pr.BAYER else (37, 11)
    n, row = 3, w * pr.BPP[pixfmt]
    imgs = _images(pixfmt, w, h, n, "noise", rng)
    sp, dp = row + 5, 3 * w + 7  # odd pitches
    simg, dimg = sp * h + 3, dp * h + 1
    src = np.full(1 + n * simg, POISON_SRC, np.uint8)
    dst = np.full(3 + n * dimg + 16, POISON_DST, np.uint8)
    for i in range(n):
        src[1 + i * simg:1 + i * simg + sp * h].reshape(h, sp)[:, :row] = imgs[i].reshape(h, row)
    st = L.vsf_to_bgr(ctx._h, src.ctypes.data + 1, n, w, h, pixfmt, simg, sp, dst.ctypes.data + 3, dimg, dp)  # odd addresses
    assert st == capi.VSF_OK
    may = np.zeros(dst.shape, bool)
    for i in range(n):
        rows = dst[3 + i * dimg:3 + i * dimg + dp * h].reshape(h, dp)
        np.testing.assert_array_equal(rows[:, :3 * w].reshape(h, w, 3), br.to_bgr(imgs[i], pixfmt))
        may[3 + i * dimg:3 + i * dimg + dp * h].reshape(h, dp)[:, :3 * w] = True
    assert (dst[~may] == POISON_DST).all(), "more than 3 w bytes of a row were written"
    np.testing.assert_array_equal(ctx.to_bgr(imgs, pixfmt), np.stack([br.to_bgr(im, pixfmt) for im in imgs]))


def test_refusals_launch_nothing(ctx):
    import torch
    from vision_slam_frontend_amd import capi
    src = torch.full((8192,), 9, dtype=torch.uint8, device="cuda:0")
    dst = torch.full((8192,), POISON_DST, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    s, d = src.data_ptr(), dst.data_ptr()
    bad = [
        dict(pixfmt=2), dict(pixfmt=15), dict(pixfmt=23), dict(pixfmt=-1),
        dict(pixfmt=pr.PIX_BGR8, sp=44),      # a source row is 48 bytes
        dict(pixfmt=pr.PIX_BGRA8, sp=60),
        dict(pixfmt=pr.PIX_BGR8, sp=50),      # not a multiple of 4
        dict(pixfmt=pr.PIX_MONO8, dp=44),     # below (3 w + 3) & ~3 = 48
        dict(pixfmt=pr.PIX_MONO8, w=15, dp=44),  # 45 bytes a row: 48 wanted
        dict(pixfmt=pr.PIX_MONO8, dp=50),
        dict(pixfmt=pr.PIX_BGR8, s=s + 1), dict(pixfmt=pr.PIX_BGR8, d=d + 2),
        dict(pixfmt=pr.PIX_BGR8, simg=64 * 3), dict(pixfmt=pr.PIX_BGR8, dimg=48 * 3), dict(pixfmt=pr.PIX_BGR8, dimg=48 * 4 + 2),
        dict(pixfmt=pr.PIX_BGR8, w=0), dict(pixfmt=pr.PIX_BGR8, h=0), dict(pixfmt=pr.PIX_BGR8, n=0), dict(pixfmt=pr.PIX_BGR8, n=65536),
        dict(pixfmt=pr.PIX_BAYER_GRBG8, w=16385, sp=16388, dp=49156, simg=16388 * 4, dimg=49156 * 4),
        dict(pixfmt=pr.PIX_BGR8, s=0), dict(pixfmt=pr.PIX_BGR8, d=0),
    ]
    for kw in bad:
        a = dict(s=s, n=1, w=16, h=4, pixfmt=0, simg=64 * 4, sp=64, d=d, dimg=48 * 4, dp=48)
        a.update(kw)
        st = ctx.to_bgr_batch_dev(a["s"], a["n"], a["w"], a["h"], a["pixfmt"], a["simg"], a["sp"], a["d"], a["dimg"], a["dp"])
        assert st == capi.VSF_ERR_INVALID_ARG, kw
    L = capi.lib()
    host_src, host_dst = np.zeros(4096, np.uint8), np.full(4096, POISON_DST, np.uint8)
    for kw in [dict(pixfmt=2), dict(sp=15), dict(dp=47), dict(w=0), dict(w=16385), dict(h=32768), dict(n=0), dict(s=0), dict(d=0)]:
        a = dict(s=host_src.ctypes.data, n=1, w=16, h=4, pixfmt=0, simg=64, sp=16, d=host_dst.ctypes.data, dimg=192, dp=48)
        a.update(kw)
        st = L.vsf_to_bgr(ctx._h, a["s"], a["n"], a["w"], a["h"], a["pixfmt"], a["simg"], a["sp"], a["d"], a["dimg"], a["dp"])
        assert st == capi.VSF_ERR_INVALID_ARG, kw
    assert ctx.sync() == capi.VSF_OK
    assert (dst.cpu().numpy() == POISON_DST).all() and (host_dst == POISON_DST).all()
