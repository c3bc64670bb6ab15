"""The references of the colour decode themselves (tests/jpeg_ref_bgr.py, tests/png_ref_bgr.py: the system's libjpeg.so.8 and
libpng16.so.16 driven as cv::imdecode(buf, IMREAD_COLOR) drives them, their structs and prototypes bound by hand): on every
committed JPEG and PNG file they must give Pillow's RGB decode with the channels swapped -- Pillow bundles a libjpeg-turbo
and a libpng of its own -- and on every crafted file of tests/test_gpu_imdecode_bgr.py they must not warn: a file that makes
libjpeg warn is no parity case, and none may drop out unseen."""
import io
from pathlib import Path

import numpy as np
import pytest
from PIL import Image

import imdecode_bgr_cases as cases_bgr
import jpeg_craft as jc
import jpeg_ref
import jpeg_ref_bgr
import png_ref_bgr

GOLDEN = Path(__file__).resolve().parent / "golden"

# Pillow reads a 16-bit gray file as mode I;16 and clips it to 255 on the way to RGB; libpng's strip_16 keeps the high byte.
# Held against the file's own samples instead (below).
PIL_DIFFERS = {"craft_gray16.png": "Pillow clips 16-bit gray samples to 255 when it converts to RGB; libpng keeps their high byte"}


def pil_bgr(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))[:, :, ::-1]


def test_libraries_are_there():
    assert jpeg_ref_bgr.available(), "no libjpeg.so.8 to build tests/cpp/jpeg_ref_bgr.c against"
    assert png_ref_bgr.available(), "no libpng16.so.16 to build tests/cpp/png_ref_bgr.c against"


@pytest.mark.parametrize("folder", ["jpeg", "jpeg_enc"])
def test_jpeg_reference_equals_pillow(folder):
    files = sorted((GOLDEN / folder).glob("*.jpg"))
    assert len(files) >= 13
    for f in files:
        data = f.read_bytes()
        st, img, warn = jpeg_ref_bgr.imdecode_bgr(data)
        assert st == 0 and warn == 0, (f.name, st, warn)
        np.testing.assert_array_equal(img, pil_bgr(data), err_msg=f.name)
        gst, gray, _ = jpeg_ref.imdecode_gray(data)
        if Image.open(io.BytesIO(data)).mode == "L":   # one component: B = G = R = Y
            np.testing.assert_array_equal(img, np.dstack([gray] * 3), err_msg=f.name)


def test_png_reference_equals_pillow():
    files = sorted((GOLDEN / "png").glob("*.png"))
    assert len(files) >= 35
    seen = set()
    for f in files:
        data = f.read_bytes()
        st, img, info = png_ref_bgr.imdecode_bgr(data)
        assert st == 0 and png_ref_bgr.warnings() == 0, (f.name, st, png_ref_bgr.last_error(), png_ref_bgr.last_warning())
        if f.name in PIL_DIFFERS:
            seen.add(f.name)
            with Image.open(io.BytesIO(data)) as im:
                high = (np.asarray(im).astype(np.uint16) >> 8).astype(np.uint8)
            np.testing.assert_array_equal(img, np.dstack([high] * 3), err_msg=f.name)
            assert not np.array_equal(img, pil_bgr(data)), "%s: %s -- no longer" % (f.name, PIL_DIFFERS[f.name])
        else:
            np.testing.assert_array_equal(img, pil_bgr(data), err_msg=f.name)
    assert seen == set(PIL_DIFFERS)


def test_crafted_files_make_libjpeg_neither_warn_nor_guess():
    """Every crafted file of the device tests: no warning; decoded (status 0) or refused while the upsamplers are set up
    (status 2: a chroma factor that does not divide the luminance's), nothing else; and where Pillow reads the file too, the
    same pixels."""
    refused = set()
    n = 0
    for name, data, w, h, factors, process in jc.sampling_cases():
        st, img, warn = jpeg_ref_bgr.imdecode_bgr(data, w, h)
        assert warn == 0 and st in (0, 2), (name, st, warn)
        fractional = len(factors) == 3 and any(factors[0][0] % fh or factors[0][1] % fv for fh, fv in factors[1:])
        assert (st == 2) == fractional, (name, st)
        if st == 2:
            refused.add(factors)
        else:
            np.testing.assert_array_equal(img, pil_bgr(data), err_msg=name)
        n += 1
    assert refused == {f for f in jc.SAMPLING_INTERLEAVED + jc.SAMPLING_SEPARATE_ONLY
                       if any(f[0][0] % fh or f[0][1] % fv for fh, fv in f[1:])} and refused
    for layout in cases_bgr.LAYOUTS:
        every = cases_bgr.upsampler_cases(layout)
        assert len(every) == len(cases_bgr.WIDTHS) * len(cases_bgr.HEIGHTS)
        for (w, h), cases in every.items():
            assert len(cases) == len(cases_bgr.RESTARTS)
            for name, data in cases:
                st, img, warn = jpeg_ref_bgr.imdecode_bgr(data, w, h)
                assert st == 0 and warn == 0, (name, st, warn)
                np.testing.assert_array_equal(img, pil_bgr(data), err_msg=name)
                n += 1
    for layout in ("444", "420"):
        name, data, w, h = cases_bgr.range_case(layout)
        st, img, warn = jpeg_ref_bgr.imdecode_bgr(data, w, h)
        assert st == 0 and warn == 0, name
        for ch in range(3):
            assert img[..., ch].min() == 0 and img[..., ch].max() == 255, (name, ch)
    assert n > 1000
