"""The gray image of a raw frame in every pixel format of include/vsf.h (VSF_PIX_*), built from the unmodified oracle.

Bayer orders need no second statement of the demosaic.  oracle.binding.bayer_bg_to_gray is OpenCV's loop for RGGB (red at
even x, even y).  A mosaic of another order has its red one column (GRBG), one row (GBRG) or both (BGGR) further along, so
with that many columns / rows of ARBITRARY bytes put in front it is an RGGB mosaic: an interior pixel (x, y) of the order's
result is pixel (x + dx, y + dy) of the oracle's result on the padded mosaic -- interior there too, and its 3 x 3
neighbourhood never reaches the bytes put in front.  That covers every interior pixel 1 .. w - 2, 1 .. h - 2; the
one-pixel frame is OpenCV's copy rule: columns first (inside rows 1 .. h - 2), then whole rows.  A side below 3: all zero.

Packed colour is RGB2Gray<uchar>: (1868 B + 9617 G + 4899 R + 8192) >> 14 on the channels the name gives, alpha ignored.
"""
import numpy as np

from oracle import binding as ob

PIX_MONO8, PIX_BAYER_RGGB8 = 0, 1
PIX_BAYER_GRBG8, PIX_BAYER_GBRG8, PIX_BAYER_BGGR8, PIX_BGR8, PIX_RGB8, PIX_BGRA8, PIX_RGBA8 = range(16, 23)

# where red sits: (x parity, y parity)
RED_SITE = {PIX_BAYER_RGGB8: (0, 0), PIX_BAYER_GRBG8: (1, 0), PIX_BAYER_GBRG8: (0, 1), PIX_BAYER_BGGR8: (1, 1)}
BAYER = tuple(RED_SITE)
COLOUR = (PIX_BGR8, PIX_RGB8, PIX_BGRA8, PIX_RGBA8)
BPP = {PIX_MONO8: 1, **{f: 1 for f in BAYER}, PIX_BGR8: 3, PIX_RGB8: 3, PIX_BGRA8: 4, PIX_RGBA8: 4}
ENCODING = {"mono8": PIX_MONO8, "bayer_rggb8": PIX_BAYER_RGGB8, "bayer_grbg8": PIX_BAYER_GRBG8,
            "bayer_gbrg8": PIX_BAYER_GBRG8, "bayer_bggr8": PIX_BAYER_BGGR8, "bgr8": PIX_BGR8, "rgb8": PIX_RGB8,
            "bgra8": PIX_BGRA8, "rgba8": PIX_RGBA8}


def bayer_to_gray(mosaic: np.ndarray, pixfmt: int, front: int = 0x5A) -> np.ndarray:
    """`front`: the byte (or an array broadcast over the padded mosaic) the prepended column / row holds."""
    m = np.ascontiguousarray(mosaic, np.uint8)
    h, w = m.shape
    out = np.zeros((h, w), np.uint8)
    if w < 3 or h < 3:
        return out
    dx, dy = RED_SITE[pixfmt]
    padded = np.empty((h + dy, w + dx), np.uint8)
    padded[...] = front
    padded[dy:, dx:] = m
    g = ob.bayer_bg_to_gray(padded)
    out[1:h - 1, 1:w - 1] = g[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    out[1:h - 1, 0] = out[1:h - 1, 1]
    out[1:h - 1, w - 1] = out[1:h - 1, w - 2]
    out[0] = out[1]
    out[h - 1] = out[h - 2]
    return out


def colour_to_gray(img: np.ndarray, pixfmt: int) -> np.ndarray:
    c = np.asarray(img, np.uint8).astype(np.uint32)
    assert c.ndim == 3 and c.shape[2] == BPP[pixfmt]
    b, r = (c[..., 2], c[..., 0]) if pixfmt in (PIX_RGB8, PIX_RGBA8) else (c[..., 0], c[..., 2])
    return ((1868 * b + 9617 * c[..., 1] + 4899 * r + 8192) >> 14).astype(np.uint8)


def to_gray(img: np.ndarray, pixfmt: int) -> np.ndarray:
    if pixfmt == PIX_MONO8:
        return np.ascontiguousarray(img, np.uint8).copy()
    if pixfmt in RED_SITE:
        return bayer_to_gray(img, pixfmt)
    return colour_to_gray(img, pixfmt)


def site_constant_mosaic(w: int, h: int, pixfmt: int, r: int, g: int, b: int) -> np.ndarray:
    """A mosaic of order `pixfmt` whose red sites all hold r, green sites g, blue sites b."""
    rx, ry = RED_SITE[pixfmt]
    y, x = np.mgrid[0:h, 0:w]
    red = ((x & 1) == rx) & ((y & 1) == ry)
    blue = ((x & 1) != rx) & ((y & 1) != ry)
    return np.where(red, r, np.where(blue, b, g)).astype(np.uint8)
