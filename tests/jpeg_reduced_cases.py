"""Test helper of the reduced-size JPEG decode: baseline gray JPEG files written from chosen QUANTISED COEFFICIENTS (Annex K
Huffman tables, a quantisation table of the caller's choosing, any image size -- the last block of a row or column is then
cropped), so that a test knows the coefficients libjpeg's reduced inverse DCTs are given.  The expected pixels always come
from the library reading the file (tests/jpeg_ref_reduced.py), never from this module."""
import numpy as np

import jpeg_craft as jc

# T.81 Annex K.3.3.2, table K.5: the luminance AC table
STD_AC_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
STD_AC_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
    0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
    0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
assert len(STD_AC_VALS) == sum(STD_AC_BITS) == 162 == len(set(STD_AC_VALS))

_SOF_AT = 2 + 4 + 65  # SOI, one DQT segment of one 8-bit table


def write_file(coef, qt, width, height):
    """coef: (ceil(height / 8), ceil(width / 8), 64) quantised values in natural order; qt: 64 values 1..255, natural order."""
    by, bx, _ = coef.shape
    assert by == -(-height // 8) and bx == -(-width // 8)
    data = bytearray(jc.write_gray_jpeg(coef, qt, (jc.STD_DC_BITS, jc.STD_DC_VALS), (STD_AC_BITS, STD_AC_VALS)))
    assert data[_SOF_AT:_SOF_AT + 5] == b"\xFF\xC0\x00\x0B\x08"
    data[_SOF_AT + 5:_SOF_AT + 9] = bytes([height >> 8, height & 255, width >> 8, width & 255])
    return bytes(data)


def _grid(width, height):
    return -(-height // 8), -(-width // 8)


def cases():
    """-> [(name, coef, qt, width, height)].  Single coefficients at each of the 64 positions (which rows and columns a form
    ignores shows here), dense random blocks under quantisers 1, 255 and mixed, blocks at the Huffman limits of a baseline file
    (DC +-2047, AC +-1023) under quantiser 255 (far beyond what 32-bit sums hold), and sizes that crop the last block."""
    rng = np.random.default_rng(20261019)
    out = []
    for dc in (0, 9):
        c = np.zeros((8, 8, 64), np.int64)
        c[..., 0] = dc
        for k in range(64):
            c[k // 8, k % 8, k] = 37 if k else 45
        out.append(("single_coefficients_dc%d" % dc, c, np.full(64, 16), 64, 64))
    c = np.zeros((8, 8, 64), np.int64)
    for k in range(64):
        c[k // 8, k % 8, k] = -1023 if k else -1000
    c[..., 0] += np.where(c[..., 0] == 0, 3, 0)
    out.append(("single_coefficients_large", c, np.full(64, 255), 64, 64))
    for name, qt in (("q1", np.ones(64, np.int64)), ("q255", np.full(64, 255)), ("qmixed", rng.integers(1, 64, 64))):
        c = rng.integers(-60, 61, (5, 7, 64))
        out.append(("dense_" + name, c, qt, 53, 39))
    # the limits: every AC term +-1023, the DC terms walking 2047, 0, -2047, 0 ... (a DC DIFFERENCE is at most 2047 in size)
    c = np.where(rng.random((4, 4, 64)) < 0.5, -1023, 1023)
    c[..., 0] = np.array([2047, 0, -2047, 0] * 4).reshape(4, 4)
    out.append(("huffman_limits_q255", c, np.full(64, 255), 32, 32))
    c = rng.integers(-1023, 1024, (3, 3, 64))
    c[..., 0] = rng.integers(-1000, 1001, (3, 3))
    out.append(("dense_wide_q255", c, np.full(64, 255), 17, 19))
    for w, h in ((1, 1), (7, 5), (9, 9), (17, 9)):
        by, bx = _grid(w, h)
        c = rng.integers(-25, 26, (by, bx, 64))
        c[..., 0] = rng.integers(-100, 101, (by, bx))
        out.append(("crop_%dx%d" % (w, h), c, rng.integers(1, 12, 64), w, h))
    return out
