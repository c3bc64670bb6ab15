"""The reduced-size decode's host half, with no context and no GPU: the size rule (vsf_reduced_size), and what a reduced
submit makes of ONE payload before anything is booked (vsf_observe_probe_compressed_reduced) -- a denominator that is not
1, 2, 4 or 8, a PNG file at a reduced size, a file of the wrong size for its denominator."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
CAP = 1 << 20


@pytest.fixture(scope="module")
def capi():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g
    from vision_slam_frontend_amd import capi
    if not capi.LIB_PATH.exists():
        g.build()
    return capi


def test_reduced_size_is_the_ceiling_for_every_denominator(capi):
    for w in range(1, 18):
        for h in (1, 2, 7, 8, 9, 16, 17):
            for d in (1, 2, 4, 8):
                assert capi.reduced_size(w, h, d) == (capi.VSF_OK, -(-w // d), -(-h // d)), (w, h, d)
    assert capi.reduced_size(65535, 65535, 8) == (capi.VSF_OK, 8192, 8192)
    for d in (0, 3, 5, 6, 16, -1, -2):
        assert capi.reduced_size(64, 48, d) == (capi.VSF_ERR_INVALID_ARG, 0, 0), d
    for w, h in ((0, 5), (5, 0), (-1, 5)):
        assert capi.reduced_size(w, h, 2) == (capi.VSF_ERR_INVALID_ARG, 0, 0)


def test_probe_applies_the_size_rule_per_file(capi):
    f = (GOLD / "jpeg" / "ycc420_71x53_q75.jpg").read_bytes()
    for d, (w, h) in ((1, (71, 53)), (2, (36, 27)), (4, (18, 14)), (8, (9, 7))):
        assert capi.probe_compressed_reduced(f, d, w, h, CAP) == (capi.VSF_OK, 1)
        assert capi.probe_compressed_reduced(f, d, w, h, CAP, force_serial=True) == (capi.VSF_OK, 1)
        for ww, hh in ((w + 1, h), (w, h - 1), (71, 53) if d > 1 else (36, 27)):
            assert capi.probe_compressed_reduced(f, d, ww, hh, CAP)[0] == capi.VSF_ERR_INVALID_ARG, (d, ww, hh)
    prog = (GOLD / "jpeg" / "prog_gray_320x240_q85.jpg").read_bytes()
    assert capi.probe_compressed_reduced(prog, 2, 160, 120, CAP) == (capi.VSF_OK, 1)
    assert capi.probe_compressed_reduced(prog, 4, 160, 120, CAP)[0] == capi.VSF_ERR_INVALID_ARG
    # the cap applies to the file as it is, before it is parsed
    assert capi.probe_compressed_reduced(prog, 2, 160, 120, len(prog) - 1)[0] == capi.VSF_ERR_CAPACITY


def test_probe_refuses_a_bad_denominator_and_a_reduced_png(capi):
    f = (GOLD / "jpeg" / "gray_64x48_noise_q80.jpg").read_bytes()
    for d in (0, 3, 16, -4):
        assert capi.probe_compressed_reduced(f, d, 64, 48, CAP)[0] == capi.VSF_ERR_INVALID_ARG, d
    png = next(p for p in sorted((GOLD / "png").glob("*.png")))
    data = png.read_bytes()
    st, w, h = _png_size(capi, data)
    assert st == capi.VSF_OK
    assert capi.probe_compressed_reduced(data, 1, w, h, CAP)[0] in (capi.VSF_OK, capi.VSF_ERR_UNSUPPORTED)
    for d in (2, 4, 8):  # whatever its size: cv::imdecode would decode it whole and call cv::resize
        rw, rh = -(-w // d), -(-h // d)
        assert capi.probe_compressed_reduced(data, d, rw, rh, CAP)[0] == capi.VSF_ERR_UNSUPPORTED, d
    assert capi.probe_compressed_reduced(b"BM" + bytes(64), 2, 8, 8, CAP)[0] == capi.VSF_ERR_UNSUPPORTED


def _png_size(capi, data):
    import ctypes as C
    import numpy as np
    b = np.frombuffer(data, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    st = capi.lib().vsf_compressed_image_size(b.ctypes.data_as(C.c_void_p), len(b), C.byref(w), C.byref(h))
    return st, w.value, h.value
