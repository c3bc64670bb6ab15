"""The reduced inverse DCTs the device decodes IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8 with (csrc/vsf_jpeg_idct_reduced.h, the
header k_jpeg.hip's kernels include) against the system's libjpeg, with no GPU: tests/jpeg_reduced_cases.py writes chosen
quantised coefficients into baseline gray files, libjpeg decodes them at scale 1/2, 1/4, 1/8 (tests/jpeg_ref_reduced.py),
and a stand-alone program (tests/cpp/test_idct_reduced.cc) applies the header's transform to the same coefficients: equal
byte for byte.  The program runs plainly and under AddressSanitizer + UBSan (stand-alone, its own main).  And the binding
itself: at d = 1 it reproduces tests/golden/jpeg/expected_gray.npz."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpeg_reduced_cases as rc
import jpeg_ref_reduced as ref

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_idct_reduced.cc"
INC = ROOT / "vision_slam_frontend_amd" / "csrc"
GOLD = ROOT / "tests" / "golden" / "jpeg"


@pytest.fixture(scope="module", autouse=True)
def _yardstick():
    """The system's libjpeg IS the yardstick of this feature: without it these tests fail, they do not skip."""
    assert ref.available(), "libjpeg.so.8 cannot be loaded: the reduced-size decode has no yardstick here"


@pytest.fixture(scope="module")
def library_pixels(_yardstick):
    """{(name, d): what libjpeg decodes}: read without a warning, of the size ceil(W / d) x ceil(H / d)."""
    out = {}
    for name, coef, qt, w, h in rc.cases():
        data = rc.write_file(coef, qt, w, h)
        for d in (2, 4, 8):
            st, img, warn = ref.imdecode_reduced_gray(data, d)
            assert st == 0 and warn == 0, (name, d, st, warn)
            assert img.shape == (-(-h // d), -(-w // d)), (name, d, img.shape)
            out[(name, d)] = img
    return out


def _run_program(exe, tmp_path):
    cases = rc.cases()
    blob = bytearray(struct.pack("<i", 3 * len(cases)))
    for name, coef, qt, w, h in cases:
        for d in (2, 4, 8):
            blob += struct.pack("<iii", d, w, h) + np.asarray(qt, "<u2").tobytes() + np.asarray(coef, "<i2").tobytes()
    src, dst = tmp_path / "cases.bin", tmp_path / "pixels.bin"
    src.write_bytes(bytes(blob))
    p = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    px = np.frombuffer(dst.read_bytes(), np.uint8)
    out, at = {}, 0
    for name, coef, qt, w, h in cases:
        for d in (2, 4, 8):
            ow, oh = -(-w // d), -(-h // d)
            out[(name, d)] = px[at:at + ow * oh].reshape(oh, ow)
            at += ow * oh
    assert at == px.size
    return out


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_header_equals_libjpeg(tmp_path, library_pixels, flags):
    exe = tmp_path / "test_idct_reduced"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(INC), "-o", str(exe), str(SRC)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = _run_program(exe, tmp_path)
    assert set(got) == set(library_pixels)
    for key, want in library_pixels.items():
        np.testing.assert_array_equal(got[key], want, err_msg="%s at 1/%d" % key)


def test_single_coefficients_show_what_each_form_ignores(library_pixels):
    """In the file of one coefficient per block (block k holds position k), libjpeg's own output is flat exactly in the blocks
    whose coefficient the form does not read: row / column 4 at 1/2; every row / column but 0, 1, 3, 5, 7 at 1/4; all but the
    DC term at 1/8.  (This pins the yardstick's meaning; test_header_equals_libjpeg pins the header to it.)"""
    for d, used in ((2, {0, 1, 2, 3, 5, 6, 7}), (4, {0, 1, 3, 5, 7}), (8, {0})):
        img = library_pixels[("single_coefficients_dc0", d)]
        s = 8 // d
        for k in range(64):
            blk = img[(k // 8) * s:(k // 8 + 1) * s, (k % 8) * s:(k % 8 + 1) * s]
            read = (k // 8) in used and (k % 8) in used
            assert (blk != 128).any() == read, (d, k, blk)


def test_binding_at_full_size_reproduces_the_golden_pixels():
    expected = np.load(GOLD / "expected_gray.npz")
    for name in sorted(expected.files):
        st, img, warn = ref.imdecode_reduced_gray((GOLD / (name + ".jpg")).read_bytes(), 1)
        assert st == 0 and warn == 0, (name, st, warn)
        np.testing.assert_array_equal(img, expected[name], err_msg=name)


def test_sizes_the_issue_states():
    """ycc420_71x53 -> 36x27, 18x14, 9x7; prog_gray_320x240 -> 160x120 at 1/2; gray_33x17 -> 9x5 at 1/4."""
    f = (GOLD / "ycc420_71x53_q75.jpg").read_bytes()
    assert [ref.imdecode_reduced_gray(f, d)[1].shape for d in (2, 4, 8)] == [(27, 36), (14, 18), (7, 9)]
    assert ref.imdecode_reduced_gray((GOLD / "prog_gray_320x240_q85.jpg").read_bytes(), 2)[1].shape == (120, 160)
    assert ref.imdecode_reduced_gray((GOLD / "gray_33x17_q95.jpg").read_bytes(), 4)[1].shape == (5, 9)
