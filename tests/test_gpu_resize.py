"""cv::resize on the device (vsf_resize_gray_batch_dev, k_resize.hip) against the oracle's general restatement
(oracle.binding.resize_linear), bit for bit -- integers on both sides, so there is no tolerance to choose.  The size pairs meet
every branch: the exact 2 x (cv::resize's INTER_AREA shortcut, also pinned by its own definition), odd floors, 3 x, 8 x,
different ratios per axis, enlargement with its clamped last taps, a copy, a destination whose last dword is partial, tiny
sizes, and -- beyond what one wave's LDS window holds -- a 40 x reduction, where every tap fetches its own dword.  Sources lie at
odd pitches and unaligned bases, the last row ending on the last byte of its tensor; destinations carry poison in their
padding that must survive."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (source w, h), (destination w, h)
PAIRS = [((128, 96), (64, 48)), ((129, 97), (64, 48)), ((192, 144), (64, 48)), ((512, 384), (64, 48)), ((100, 80), (64, 48)),
         ((40, 30), (64, 48)), ((64, 48), (64, 48)), ((131, 67), (61, 47)), ((7, 5), (3, 2)), ((7, 5), (1, 1)),
         # more than one wave per row with a partial last wave, at 2.5 x (3 dwords per lane) and 5 x (10 per lane)
         ((1300, 40), (520, 16)), ((2600, 24), (520, 10)),
         # a span no LDS window holds: every tap on its own
         ((10400, 9), (260, 4)),
         # enlargement of a wide row: more than one wave, spans of a few pixels
         ((130, 9), (523, 20))]
IDS = ["%dx%d-%dx%d" % (s + d) for s, d in PAIRS]
POISON = 0xA5


def _images(n, w, h, seed):
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, 256, (h, w), dtype=np.uint8)]
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(((xx * 255) // max(w - 1, 1)).astype(np.uint8))
    out.append(((yy * 3 + xx * 7) % 256).astype(np.uint8))
    while len(out) < n:
        out.append(rng.integers(0, 256, (h, w), dtype=np.uint8))
    return out[:n]


def _want(images, dw, dh):
    from oracle import binding as ob
    return [ob.resize_linear(im, dw, dh) for im in images]


def _to_device(images, offset, pitch):
    """The images in ONE tensor: image i at offset + i * stride, rows `pitch` apart, everything else poisoned; the last row of
    the last image ends on the tensor's last byte."""
    import torch
    h, w = images[0].shape
    stride = h * pitch
    host = np.full(offset + (len(images) - 1) * stride + (h - 1) * pitch + w, POISON, np.uint8)
    for i, im in enumerate(images):
        np.lib.stride_tricks.as_strided(host[offset + i * stride:], (h, w), (pitch, 1))[:] = im
    return torch.from_numpy(host).to("cuda:0"), stride


def _run(ctx, images, dw, dh, offset, src_pitch, dst_pitch):
    import torch
    from vision_slam_frontend_amd import capi
    h, w = images[0].shape
    n = len(images)
    src, src_stride = _to_device(images, offset, src_pitch)
    assert src.data_ptr() % 4 == 0
    dst_stride = dh * dst_pitch + 5
    dst = torch.full((n * dst_stride,), POISON, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.resize_gray_batch_dev(src.data_ptr() + offset, n, w, h, src_stride, src_pitch, dst.data_ptr(), dw, dh, dst_stride, dst_pitch)
    assert ctx.sync() == capi.VSF_OK
    out = dst.cpu().numpy().reshape(n, dst_stride)
    got = [np.lib.stride_tricks.as_strided(o, (dh, dw), (dst_pitch, 1)).copy() for o in out]
    # everything that is no pixel of a destination image is as it was
    mask = np.ones((n, dst_stride), bool)
    for i in range(n):
        np.lib.stride_tricks.as_strided(mask[i], (dh, dw), (dst_pitch, 1))[:] = False
    assert (out[mask] == POISON).all(), "bytes outside the destination images were written"
    return got


@pytest.fixture(scope="module")
def ctx():
    from vision_slam_frontend_amd import capi
    with capi.Context(capi.default_params(64, 64, max_images=2, nfeatures=100)) as c:  # (its own size plays no part)
        yield c


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_resize_equals_the_oracle(ctx, pair):
    """n = 5 (seeded random, gradients) and n = 1; source base offsets 1, 2, 3 with odd pitches; destination pitches: the width
    itself, an odd one (rows that begin on no dword: byte stores) and a multiple of 4 larger than the width (dword stores,
    the last one partial where the width is no multiple of 4)."""
    (sw, sh), (dw, dh) = pair
    images = _images(5, sw, sh, seed=sw * 7 + dw)
    want = _want(images, dw, dh)
    dst_pitches = (dw, (dw + 3) | 1, ((dw + 3) & ~3) + 8)
    for k, offset in enumerate((1, 2, 3)):
        got = _run(ctx, images, dw, dh, offset, (sw + 2 * k) | 1, dst_pitches[k])
        for i in range(5):
            assert np.array_equal(got[i], want[i]), "image %d differs at offset %d" % (i, offset)
    got = _run(ctx, images[:1], dw, dh, 0, sw, dst_pitches[2])
    assert np.array_equal(got[0], want[0])


def test_exact_half_is_the_area_average(ctx):
    """cv::resize switches to INTER_AREA at an exact 2 x reduction in both axes; its fast path is (a + b + c + d + 2) >> 2."""
    images = _images(5, 128, 96, seed=11)
    got = _run(ctx, images, 64, 48, 3, 131, 64)
    for im, g in zip(images, got):
        v = im.astype(np.int32)
        area = (v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2
        assert np.array_equal(g, area.astype(np.uint8))


def test_refusals_launch_nothing(ctx):
    import torch
    from vision_slam_frontend_amd import capi
    src = torch.zeros(5 * 96 * 128, dtype=torch.uint8, device="cuda:0")
    dst = torch.full((5 * 48 * 64,), POISON, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    s, d = src.data_ptr(), dst.data_ptr()
    ok = dict(d_src=s, n_images=5, src_width=128, src_height=96, src_image_stride=96 * 128, src_row_stride=128, d_dst=d,
              dst_width=64, dst_height=48, dst_image_stride=48 * 64, dst_row_stride=64)
    bad = [dict(d_src=0), dict(d_dst=0), dict(n_images=0), dict(n_images=-1), dict(src_width=0), dict(src_height=0),
           dict(dst_width=0), dict(dst_height=0), dict(src_width=32768, src_row_stride=32768), dict(src_height=32768),
           dict(dst_width=32768, dst_row_stride=32768), dict(dst_height=32768), dict(src_row_stride=127),
           dict(dst_row_stride=63), dict(src_image_stride=95 * 128 + 127), dict(dst_image_stride=47 * 64 + 63)]
    for change in bad:
        st = ctx.resize_gray_batch_dev(**{**ok, **change}, allow_status=(capi.VSF_ERR_INVALID_ARG,))
        assert st == capi.VSF_ERR_INVALID_ARG, change
        assert ctx.sync() == capi.VSF_OK
    assert (dst.cpu().numpy() == POISON).all()
    # ... and the call they were cut from is fine
    assert ctx.resize_gray_batch_dev(**ok) == capi.VSF_OK and ctx.sync() == capi.VSF_OK
    assert (dst.cpu().numpy() == 0).all()
