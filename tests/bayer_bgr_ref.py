"""The B G R image of a raw frame in every pixel format of include/vsf.h (VSF_PIX_*): what src/test/bag_extract.cc:75-88 puts
between cv::imdecode and cv::imwrite, restated in numpy.

Mosaics: cv::cvtColor(COLOR_Bayer??2BGR) of OpenCV 3.2, imgproc/demosaicing.cpp Bayer2RGB_<uchar> with three destination
channels.  Stated once, for RGGB (OpenCV's BayerBG: red at even x, even y; blue at odd, odd).  With the 3 x 3 neighbourhood of an
interior pixel
    cross = (N + S + W + E + 2) >> 2,  diag = (NW + NE + SW + SE + 2) >> 2,  hor = (W + E + 1) >> 1,  ver = (N + S + 1) >> 1
    red / blue site:  own colour = centre, G = cross, the other colour = diag
    green site:       G = centre, the colour of the row's sites = hor, the other = ver.
The three other orders take the shift of tests/pixfmt_ref.py: a mosaic whose red is one column (GRBG), one row (GBRG) or both
(BGGR) further along is an RGGB mosaic once that many columns / rows of ARBITRARY bytes stand in front of it; an interior pixel's
neighbourhood never reaches them.  The one-pixel frame copies its inner neighbour, columns first (inside rows 1 .. h - 2), then
whole rows.  A side below 3: all zero.  tests/test_bayer_bgr_ref.py pins this against the unmodified oracle.

Packed formats: what cv_bridge makes of them for a "bgr8" request -- MONO8: B = G = R (GRAY2BGR); BGR8: a copy; RGB8: R and B
exchanged; BGRA8 / RGBA8: alpha dropped.
"""
import numpy as np

import pixfmt_ref as pr


def _rggb_interior(m: np.ndarray) -> np.ndarray:
    """(h - 2, w - 2, 3) B G R of the interior pixels of an RGGB mosaic (h, w >= 3)."""
    p = m.astype(np.int32)
    h, w = p.shape
    c = p[1:h - 1, 1:w - 1]
    n, s, we, e = p[0:h - 2, 1:w - 1], p[2:h, 1:w - 1], p[1:h - 1, 0:w - 2], p[1:h - 1, 2:w]
    nw, ne, sw, se = p[0:h - 2, 0:w - 2], p[0:h - 2, 2:w], p[2:h, 0:w - 2], p[2:h, 2:w]
    cross, diag = (n + s + we + e + 2) >> 2, (nw + ne + sw + se + 2) >> 2
    hor, ver = (we + e + 1) >> 1, (n + s + 1) >> 1
    y, x = np.mgrid[1:h - 1, 1:w - 1]
    ex, ey = (x & 1) == 1, (y & 1) == 1
    red, blue = ~ex & ~ey, ex & ey
    g = np.where(red | blue, cross, c)
    b = np.where(blue, c, np.where(red, diag, np.where(ey, hor, ver)))  # green site of a blue row (odd y): blue lies W / E
    r = np.where(red, c, np.where(blue, diag, np.where(ey, ver, hor)))
    return np.stack([b, g, r], axis=-1).astype(np.uint8)


def bayer_to_bgr(mosaic: np.ndarray, pixfmt: int, front=0x5A) -> np.ndarray:
    """`front`: the byte (or an array broadcast over the padded mosaic) the prepended column / row holds."""
    m = np.ascontiguousarray(mosaic, np.uint8)
    h, w = m.shape
    out = np.zeros((h, w, 3), np.uint8)
    if w < 3 or h < 3:
        return out
    dx, dy = pr.RED_SITE[pixfmt]
    padded = np.empty((h + dy, w + dx), np.uint8)
    padded[...] = front
    padded[dy:, dx:] = m
    inner = _rggb_interior(padded)  # [j, i] is padded pixel (i + 1, j + 1)
    out[1:h - 1, 1:w - 1] = inner[dy:dy + h - 2, dx:dx + w - 2]
    out[1:h - 1, 0] = out[1:h - 1, 1]
    out[1:h - 1, w - 1] = out[1:h - 1, w - 2]
    out[0] = out[1]
    out[h - 1] = out[h - 2]
    return out


def packed_to_bgr(img: np.ndarray, pixfmt: int) -> np.ndarray:
    c = np.ascontiguousarray(img, np.uint8)
    if pixfmt == pr.PIX_MONO8:
        assert c.ndim == 2
        return np.repeat(c[..., None], 3, axis=-1)
    assert c.ndim == 3 and c.shape[2] == pr.BPP[pixfmt]
    if pixfmt in (pr.PIX_RGB8, pr.PIX_RGBA8):
        return np.ascontiguousarray(c[..., [2, 1, 0]])
    return np.ascontiguousarray(c[..., :3])


def to_bgr(img: np.ndarray, pixfmt: int) -> np.ndarray:
    if pixfmt in pr.RED_SITE:
        return bayer_to_bgr(img, pixfmt)
    return packed_to_bgr(img, pixfmt)


def bgr_to_gray(bgr: np.ndarray) -> np.ndarray:
    """color.cpp RGB2Gray<uchar> on B G R."""
    c = np.asarray(bgr, np.uint8).astype(np.uint32)
    return ((1868 * c[..., 0] + 9617 * c[..., 1] + 4899 * c[..., 2] + 8192) >> 14).astype(np.uint8)
