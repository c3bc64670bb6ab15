"""tests/bayer_bgr_ref.py -- the numpy restatement of cvtColor(COLOR_Bayer??2BGR) the GPU tests of vsf_to_bgr_batch_dev and
vsf_bag_extract_batch compare with -- pinned against the unmodified oracle: RGB2Gray of its output is
oracle.binding.bayer_bg_to_gray (through tests/pixfmt_ref.py for the three other orders), byte for byte, at every size of the
GPU tests.  The gray map is many to one, so mosaics in which only ONE colour's sites are non-zero make each channel carry the
gray alone, and site-constant mosaics must give that constant colour at every pixel, the frame included."""
import itertools

import numpy as np
import pytest

import bayer_bgr_ref as br
import pixfmt_ref as pr

SIZES = [(3, 3), (4, 3), (5, 4), (255, 17), (256, 16), (257, 33), (260, 18), (513, 5), (2, 2), (2, 5)]


def _site_mask(w, h, pixfmt, which):
    v = [0, 0, 0]
    v[which] = 1
    return pr.site_constant_mosaic(w, h, pixfmt, *v).astype(bool)


@pytest.mark.parametrize("w,h", SIZES)
def test_gray_of_the_restatement_is_the_oracle(oracle, w, h):
    rng = np.random.default_rng(w * 1009 + h)
    m = rng.integers(0, 256, (h, w), dtype=np.uint8)
    np.testing.assert_array_equal(br.bgr_to_gray(br.bayer_to_bgr(m, pr.PIX_BAYER_RGGB8)), oracle.bayer_bg_to_gray(m))
    for pixfmt in pr.BAYER:
        np.testing.assert_array_equal(br.bgr_to_gray(br.bayer_to_bgr(m, pixfmt)), pr.bayer_to_gray(m, pixfmt), err_msg=str(pixfmt))


@pytest.mark.parametrize("w,h", SIZES)
def test_each_channel_alone_carries_the_gray(oracle, w, h):
    # only one colour's sites hold noise: the two other channels are zero everywhere, so gray = (k * channel + 8192) >> 14 with
    # that colour's weight -- and a channel stored in another's place changes the weight
    rng = np.random.default_rng(w * 31 + h)
    for pixfmt in pr.BAYER:
        for which, weight in ((0, 4899), (1, 9617), (2, 1868)):  # red, green, blue sites
            m = np.where(_site_mask(w, h, pixfmt, which), rng.integers(1, 256, (h, w)), 0).astype(np.uint8)
            bgr = br.bayer_to_bgr(m, pixfmt)
            ch = 2 - which  # B G R
            others = [c for c in range(3) if c != ch]
            assert not bgr[..., others].any(), (pixfmt, which)
            want = pr.bayer_to_gray(m, pixfmt)
            np.testing.assert_array_equal((weight * bgr[..., ch].astype(np.uint32) + 8192) >> 14, want)
            if w >= 3 and h >= 3:
                assert bgr[..., ch].any()


@pytest.mark.parametrize("pixfmt", pr.BAYER)
def test_site_constant_mosaics_give_the_constant_colour(oracle, pixfmt):
    # every bilinear sum of equal values is that value: (v + v + 1) >> 1 = (4 v + 2) >> 2 = v; the five values are the ends, the
    # middle and its neighbours, where a wrong rounding or a wrong divisor shows
    for w, h in [(3, 3), (5, 4), (260, 18)]:
        for r, g, b in itertools.product((0, 1, 127, 128, 255), repeat=3):
            bgr = br.bayer_to_bgr(pr.site_constant_mosaic(w, h, pixfmt, r, g, b), pixfmt)
            assert (bgr == np.array([b, g, r], np.uint8)).all(), (w, h, r, g, b)


def test_one_colour_at_255_takes_the_five_values(oracle):
    # blue sites at 255, everything else 0, inside the image: B is 255 at a blue site, 128 beside or above / below one
    # ((255 + 1) >> 1), 255 diagonal to four ((1020 + 2) >> 2); with ONE blue site, 64 diagonal to it ((255 + 2) >> 2), 0 elsewhere
    m = np.zeros((7, 7), np.uint8)
    m[3, 3] = 255  # (odd, odd): a blue site of RGGB
    b = br.bayer_to_bgr(m, pr.PIX_BAYER_RGGB8)[..., 0]
    assert b[3, 3] == 255 and b[3, 2] == b[3, 4] == b[2, 3] == b[4, 3] == 128 and b[2, 2] == b[4, 4] == b[2, 4] == b[4, 2] == 64
    assert b.sum() == 255 + 4 * 128 + 4 * 64
    np.testing.assert_array_equal(br.bgr_to_gray(br.bayer_to_bgr(m, pr.PIX_BAYER_RGGB8)), oracle.bayer_bg_to_gray(m))


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (2, 5), (5, 2), (1, 7)])
def test_a_side_below_three_is_zero(w, h):
    m = np.full((h, w), 255, np.uint8)
    for pixfmt in pr.BAYER:
        assert not br.bayer_to_bgr(m, pixfmt).any()


def test_front_bytes_have_no_influence():
    m = np.random.default_rng(5).integers(0, 256, (18, 33), dtype=np.uint8)
    for pixfmt in pr.BAYER:
        np.testing.assert_array_equal(br.bayer_to_bgr(m, pixfmt, 0), br.bayer_to_bgr(m, pixfmt, 255))


def test_packed_conversions():
    rng = np.random.default_rng(9)
    g = rng.integers(0, 256, (4, 5), dtype=np.uint8)
    c3 = rng.integers(0, 256, (4, 5, 3), dtype=np.uint8)
    c4 = rng.integers(0, 256, (4, 5, 4), dtype=np.uint8)
    assert (br.to_bgr(g, pr.PIX_MONO8) == g[..., None]).all() and br.to_bgr(g, pr.PIX_MONO8).shape == (4, 5, 3)
    np.testing.assert_array_equal(br.to_bgr(c3, pr.PIX_BGR8), c3)
    np.testing.assert_array_equal(br.to_bgr(c3, pr.PIX_RGB8), c3[..., ::-1])
    np.testing.assert_array_equal(br.to_bgr(c4, pr.PIX_BGRA8), c4[..., :3])
    np.testing.assert_array_equal(br.to_bgr(c4, pr.PIX_RGBA8), c4[..., 2::-1])
    for f, img in ((pr.PIX_BGR8, c3), (pr.PIX_RGB8, c3), (pr.PIX_BGRA8, c4), (pr.PIX_RGBA8, c4)):
        np.testing.assert_array_equal(br.bgr_to_gray(br.to_bgr(img, f)), pr.to_gray(img, f))
