"""The crafted JPEG files of the colour-decode tests (tests/test_gpu_imdecode_bgr.py on the device, tests/test_imdecode_bgr_refs.py
for what the reference makes of them), written once per process with tests/jpeg_craft.py's writers."""
import numpy as np

import jpeg_craft as jc

LAYOUTS = {"420": ((2, 2), (1, 1), (1, 1)), "422": ((2, 1), (1, 1), (1, 1)), "440": ((1, 2), (1, 1), (1, 1)),
           "411": ((4, 1), (1, 1), (1, 1)), "444": ((1, 1), (1, 1), (1, 1))}
# component rows of 1, 2, 3 and 4 samples (jdsample.c takes its triangle filters from 3 on); a block and an MCU seam
WIDTHS = (1, 2, 3, 4, 5, 6, 7, 16, 17, 33)
# the top and the bottom row, and the context rows across MCU-row seams
HEIGHTS = (1, 2, 8, 9, 16, 17, 33)
RESTARTS = (0, "mcu", "row")   # no restart intervals, intervals of one MCU, of one MCU row

_cache = {}


def upsampler_file(rng, w, h, factors, restart):
    """One interleaved scan of `factors` at w x h from fresh random coefficients."""
    hmax, vmax = factors[0]
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    comps = [(fh, fv, rng.integers(1, 5, 64), jc.random_coefficients(rng, my * fv, mx * fh)) for fh, fv in factors]
    ri = {0: 0, "mcu": 1, "row": mx}[restart]
    return jc.write_multiscan_sequential_jpeg(w, h, comps, [(0, 1, 2)], restart_interval=ri)


def upsampler_cases(layout):
    """-> {(w, h): [(name, bytes)]}: the layout at every width and height above, with each kind of restart interval."""
    if layout not in _cache:
        rng = np.random.default_rng(sum(layout.encode()))
        _cache[layout] = {(w, h): [("%s_%dx%d_%s" % (layout, w, h, r), upsampler_file(rng, w, h, LAYOUTS[layout], r)) for r in RESTARTS]
                          for h in HEIGHTS for w in WIDTHS}
    return _cache[layout]


def range_case(layout):
    """64 x 32: DC coefficients at both ends of what 8-bit samples can be, in every combination over the MCUs (bit c of the
    MCU's number: component c at the top or at the bottom), a little AC on top -- R = Y + 1.402 (Cr - 128) and the other two
    channels leave [0, 255] on both sides.  -> (name, bytes, w, h)"""
    factors = LAYOUTS[layout]
    w, h = 64, 32
    hmax, vmax = factors[0]
    mx, my = w // (8 * hmax), h // (8 * vmax)
    rng = np.random.default_rng(7)
    comps = []
    for c, (fh, fv) in enumerate(factors):
        coef = np.zeros((my * fv, mx * fh, 64), np.int64)
        by, bx = np.indices(coef.shape[:2])
        mcu = (by // fv) * mx + (bx // fh)
        coef[..., 0] = np.where((mcu >> c) & 1, 1016, -1024)
        coef[..., 1] = rng.integers(-3, 4, coef.shape[:2])
        comps.append((fh, fv, np.ones(64, np.int64), coef))
    return "range_" + layout, jc.write_multiscan_sequential_jpeg(w, h, comps, [(0, 1, 2)]), w, h
