"""The host half of the JPEG encoder (csrc/vsf_jpeg_enc_host.cc: quality -> quantisation tables, every byte from SOI to the end
of the SOS header, the size bound) against the system's libjpeg driven as cv::imencode(".jpg") of OpenCV 3.2 drives it
(tests/jpeg_enc_ref.py) -- byte for byte, no device involved -- and the same under AddressSanitizer / UBSan (`make asan`, as
tests/test_jpeg_host_asan.py runs the parser).  Also: the fixed inputs of the GPU tests hold the features they are named for, and
the committed files of tests/golden/jpeg_enc are what the library of THIS machine writes."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import jpeg_enc_ref as ref  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vision_slam_frontend_amd" / "csrc"
ASAN_LIB = ROOT / "vision_slam_frontend_amd" / "libvsf_jpeg_host_asan.so"

if not ref.available():  # (the library is part of the image)
    pytest.skip("libjpeg.so.8 cannot be loaded", allow_module_level=True)

HEADER_QUALITIES = [1, 50, 75, 95, 100]
HEADER_SIZES = [(1, 1), (8, 8), (17, 9), (640, 480)]


def _noise(w, h, ch):
    return np.random.default_rng(w * 131 + h * 7 + ch).integers(0, 256, (h, w) if ch == 1 else (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("quality", HEADER_QUALITIES)
def test_header_equals_libjpegs(quality, channels):
    from vision_slam_frontend_amd import capi
    for w, h in HEADER_SIZES:
        want = ref.imencode(_noise(w, h, channels), quality)
        want = want[:ref.header_length(want)]
        got = capi.jpeg_encode_header(w, h, channels, quality)
        assert got == want, (w, h, len(got), len(want))
    assert capi.jpeg_encode_header(17, 9, channels, 0) == capi.jpeg_encode_header(17, 9, channels, 95)  # 0 means 95


@pytest.mark.parametrize("channels", [1, 3])
def test_capacity_holds_noise_at_quality_100(channels):
    """Quantisers of 1: the longest codes and the most stuffed bytes a file of that size can have in practice."""
    from vision_slam_frontend_amd import capi
    for w, h in HEADER_SIZES:
        f = ref.imencode(_noise(w, h, channels), 100)
        cap = capi.jpeg_encode_capacity(w, h, channels)
        assert cap >= len(f), (w, h, cap, len(f))
        # ... and an image of saturated noise (0 / 255 only: larger coefficients still)
        g = ref.imencode((_noise(w, h, channels) >> 7) * 255, 100)
        assert cap >= len(g), (w, h, cap, len(g))
    for bad in ((0, 1, 1), (1, 0, 1), (65536, 1, 1), (1, 65536, 3), (8, 8, 2), (8, 8, 4)):
        assert capi.jpeg_encode_capacity(*bad) == 0
    assert capi.jpeg_encode_capacity(65535, 65535, 3) > 2 ** 32  # (a size_t, not an int)


def test_header_call_checks_its_arguments():
    import ctypes as C
    from vision_slam_frontend_amd import capi
    L = capi.lib()
    buf = np.zeros(640, np.uint8)
    n = C.c_size_t()
    p = buf.ctypes.data_as(C.c_void_p)
    for w, h, ch, q in ((0, 8, 1, 95), (8, 0, 1, 95), (65536, 8, 1, 95), (8, 8, 2, 95), (8, 8, 1, 101), (8, 8, 1, -1)):
        assert L.vsf_debug_jpeg_encode_header(w, h, ch, q, p, 640, C.byref(n)) == capi.VSF_ERR_INVALID_ARG
    assert L.vsf_debug_jpeg_encode_header(8, 8, 3, 95, p, 622, C.byref(n)) == capi.VSF_ERR_CAPACITY and n.value == 623
    assert not buf.any()
    assert L.vsf_debug_jpeg_encode_header(8, 8, 3, 95, p, 623, C.byref(n)) == capi.VSF_OK and buf[622] == 0 and buf[621] == 63


def test_named_inputs_hold_their_features():
    """Counted in libjpeg's own output (jpeg_enc_ref.scan_stats), at the sizes and qualities the GPU tests use."""
    for ch in (1, 3):
        s = ref.scan_stats(ref.imencode(ref.make_input("noise", 64, 48, ch), 100))
        assert s["stuffed"] >= 1, s                                 # FF 00
        s = ref.scan_stats(ref.imencode(ref.make_input("noise", 33, 31, ch), 100))
        assert s["stuffed"] >= 1, s
        s = ref.scan_stats(ref.imencode(ref.make_input("checker", 16, 16, ch), 100))
        assert s["max_size"] >= 10, s                               # the top size categories
        for (w, h) in ((8, 8), (17, 9), (64, 48)):
            s = ref.scan_stats(ref.imencode(ref.make_input("zz63", w, h, ch), 50))
            assert s["max_zrl_run"] == 3 and s["zrl"] >= 3, s       # 62 zeros in front of coefficient 63: three ZRLs in a row
        for c in ("flat0", "flat128", "flat255"):
            s = ref.scan_stats(ref.imencode(ref.make_input(c, 33, 31, ch), 95))
            assert s["eob"] == s["blocks"] and s["zrl"] == 0, (c, s)  # EOB only
        s = ref.scan_stats(ref.imencode(ref.make_input("flat0", 33, 31, ch), 95))
        assert s["max_size"] >= 10, s                               # ... with a DC difference of -1024 in front
    # 4:2:0 at a width of 17: the MCUs hold blocks the luminance component does not have
    s = ref.scan_stats(ref.imencode(ref.make_input("stripes", 17, 9, 3), 95))
    assert s["blocks"] == 12, s
    a = ref.make_input("stripes", 17, 9, 3)
    assert set(np.unique(a)) == {0, 255} and (a.sum(-1) == 255).all()  # saturated primaries


def test_committed_goldens_are_what_this_libjpeg_writes():
    cases = ref.golden_cases()
    assert len(cases) >= 12 and len(list(ref.GOLDEN.glob("*.jpg"))) == len(cases)
    for name, content, w, h, ch, q in cases:
        assert (ref.GOLDEN / (name + ".jpg")).read_bytes() == ref.imencode(ref.make_input(content, w, h, ch), q), name


DRIVER = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import jpeg_enc_ref as ref
L = C.CDLL(sys.argv[1])
L.vsf_jpeg_encode_capacity.restype = C.c_size_t
L.vsf_jpeg_encode_capacity.argtypes = [C.c_int] * 3
L.vsf_debug_jpeg_encode_header.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
checked = 0
for q in (0, 1, 2, 25, 49, 50, 51, 75, 95, 99, 100):
    for ch in (1, 3):
        for w, h in ((1, 1), (8, 8), (17, 9), (640, 480), (65535, 65535), (65535, 1)):
            n = C.c_size_t()
            full = np.zeros(640, np.uint8)
            assert L.vsf_debug_jpeg_encode_header(w, h, ch, q, full.ctypes.data, 640, C.byref(n)) == 0
            exact = np.zeros(n.value, np.uint8)  # a heap buffer of exactly the header's size: a byte more is an overflow
            assert L.vsf_debug_jpeg_encode_header(w, h, ch, q, exact.ctypes.data, n.value, C.byref(n)) == 0
            assert exact.tobytes() == full[:n.value].tobytes()
            short = np.zeros(max(n.value - 1, 1), np.uint8)
            assert L.vsf_debug_jpeg_encode_header(w, h, ch, q, short.ctypes.data, n.value - 1, C.byref(n)) == 2
            if w <= 640:
                want = ref.imencode(np.zeros((h, w) if ch == 1 else (h, w, 3), np.uint8), q or 95)
                assert exact.tobytes() == want[:ref.header_length(want)], (q, ch, w, h)
            assert L.vsf_jpeg_encode_capacity(w, h, ch) > n.value
            checked += 1
for bad in ((0, 0, 0, 0), (-1, 5, 1, 50), (5, -1, 3, 50), (1 << 30, 1 << 30, 3, 50), (8, 8, 1, 1000), (8, 8, 1, -(1 << 31))):
    n = C.c_size_t()
    buf = np.zeros(640, np.uint8)
    assert L.vsf_debug_jpeg_encode_header(*bad, buf.ctypes.data, 640, C.byref(n)) == 1
    if not 1 <= bad[0] <= 65535:
        assert L.vsf_jpeg_encode_capacity(*bad[:3]) == 0
print("done checked=%d" % checked)
'''


def test_host_half_under_asan_and_ubsan(tmp_path):
    asan_rt = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    ubsan_rt = subprocess.run(["gcc", "-print-file-name=libubsan.so"], capture_output=True, text=True).stdout.strip()
    if not (asan_rt and Path(asan_rt).exists() and ubsan_rt and Path(ubsan_rt).exists()):
        pytest.skip("no sanitizer runtime in this toolchain")
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "asan"], capture_output=True, text=True)
    assert r.returncode == 0 and ASAN_LIB.exists(), r.stderr[-2000:]
    script = tmp_path / "drive.py"
    script.write_text(DRIVER)
    env = dict(os.environ, LD_PRELOAD="%s %s" % (asan_rt, ubsan_rt),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([sys.executable, str(script), str(ASAN_LIB), str(Path(__file__).resolve().parent)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-4000:])
    assert p.stdout.strip().splitlines()[-1].startswith("done checked=132"), p.stdout[-500:]
