"""The host half of the PNG encoder (csrc/vsf_png_enc_host.cc: signature, IHDR, libpng's window rule for the zlib header, the
size bound) and the encoder's CPU model (the per-block code the kernels run, driven serially) against the system's libpng driven
as cv::imencode(".png") of OpenCV 3.2 drives it (tests/png_enc_ref.py) -- byte for byte, no device involved -- and the same under
AddressSanitizer / UBSan.  Also: the reference binding equals the zlib model, the named inputs of the GPU tests hold the features
they are named for, and the committed files of tests/golden/png_enc are what the library of THIS machine writes."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import png_enc_ref as ref  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vision_slam_frontend_amd" / "csrc"
ASAN_LIB = ROOT / "vision_slam_frontend_amd" / "libvsf_jpeg_host_asan.so"

if not ref.available():  # (the library is part of the image)
    pytest.skip("libpng16.so.16 cannot be loaded", allow_module_level=True)

GRID = [(1, 1), (1, 5), (2, 1), (3, 3), (7, 5), (33, 31), (64, 48), (128, 126), (128, 127), (128, 128), (300, 200), (640, 480)]


def _noise(w, h, ch):
    return np.random.default_rng(w * 131 + h * 7 + ch).integers(0, 256, (h, w) if ch == 1 else (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("channels", [1, 3])
def test_header_equals_libpngs(channels):
    from vision_slam_frontend_amd import capi
    for w, h in GRID:
        want = ref.imencode(_noise(w, h, channels))
        got = capi.png_encode_header(w, h, channels)
        assert len(got) == 35 and got[:33] == want[:33], (w, h)
        assert want[37:41] == b"IDAT" and got[33:] == want[41:43], (w, h, got[33:].hex(), want[41:43].hex())


def test_window_bits_on_both_sides_of_16384_bytes():
    """Rows of 129 bytes: 126 rows are 16254 bytes and 127 rows 16383 (libpng shrinks the window: CINFO 6), 128 rows 16512 (the
    full window, 78 01); both bytes against the library below."""
    from vision_slam_frontend_amd import capi
    assert capi.png_encode_header(128, 126, 1)[33] == 0x68
    assert capi.png_encode_header(128, 127, 1)[33] == 0x68
    assert capi.png_encode_header(128, 128, 1)[33:] == b"\x78\x01"
    assert capi.png_encode_header(64, 48, 1)[33:] == b"\x48\x0d"
    for w, h in ((128, 126), (128, 127), (128, 128), (16383, 1), (16384, 1), (5461, 1)):
        for ch in (1, 3):
            assert capi.png_encode_header(w, h, ch)[33:] == ref.imencode(np.zeros((h, w) if ch == 1 else (h, w, 3), np.uint8))[41:43]


@pytest.mark.parametrize("channels", [1, 3])
def test_capacity_holds_noise(channels):
    from vision_slam_frontend_amd import capi
    for w, h in GRID:
        f = ref.imencode(_noise(w, h, channels))
        assert capi.png_encode_capacity(w, h, channels) >= len(f), (w, h)
    for bad in ((0, 1, 1), (1, 0, 1), (65536, 1, 1), (1, 65536, 3), (8, 8, 2), (8, 8, 4)):
        assert capi.png_encode_capacity(*bad) == 0
    assert capi.png_encode_capacity(65535, 65535, 3) > 2 ** 32  # (a size_t, not an int)


def test_reference_binding_equals_the_zlib_model():
    for ch in (1, 3):
        for w, h in GRID:
            for c in ("flat7", "noise", "few3", "ramp"):
                img = ref.make_input(c, w, h, ch)
                assert ref.imencode(img) == ref.model(img), (c, w, h, ch)
    import zlib
    assert zlib.decompress(ref.idat(ref.imencode(np.full((1, 1), 9, np.uint8)))) == b"\x00\x09"  # one pixel wide: filter type 0
    assert zlib.decompress(ref.idat(ref.imencode(np.full((5, 1), 9, np.uint8))))[::2] == bytes(5)
    assert zlib.decompress(ref.idat(ref.imencode(np.full((1, 2), 9, np.uint8)))) == b"\x01\x09\x00"  # otherwise Sub
    assert ref.filtered(np.zeros((5, 1), np.uint8))[0] == 0 and ref.filtered(np.zeros((1, 2), np.uint8))[0] == 1


def _cases():
    out = []
    for ch in (1, 3):
        for w, h in ref.SIZES:
            for c in ("flat0", "noise", "few2", "few4", "ramp"):
                if w * h > 70000 and c != "few4":
                    continue
                out.append(("%s_%dx%d_%d" % (c, w, h, ch), ref.make_input(c, w, h, ch)))
    out += [("runs", ref.make_input("runs", 2200, 3, 1)), ("filterbyte", ref.make_input("filterbyte", 64, 48, 1)),
            ("channels", ref.make_input("channels", 33, 31, 3))]
    out += [("symbols_%d" % t, ref.with_symbols(t)) for t in (16382, 16383, 16384, 16385)]
    out += [("stream_%d" % t, ref.with_stream_length(t)) for t in (8191, 8192, 8193)]
    return out


def test_cpu_model_equals_libpng():
    """The per-block code of the kernels (trees.c restated), driven serially on the CPU."""
    from vision_slam_frontend_amd import capi
    for name, img in _cases():
        assert capi.png_encode_cpu(img) == ref.imencode(img), name


def test_cpu_model_repairs_overlong_codes():
    """Frequencies that grow like Fibonacci numbers give a Huffman tree deeper than 15: gen_bitlen's overflow branch."""
    from vision_slam_frontend_amd import capi
    fib = [1, 1]
    while sum(fib) < 12000:
        fib.append(fib[-1] + fib[-2])
    vals = np.concatenate([np.full(f, 3 + 5 * i, np.uint8) for i, f in enumerate(fib)])
    np.random.default_rng(3).shuffle(vals)
    vals = vals[:(len(vals) // 127) * 127].reshape(-1, 127)
    img = ref.from_filtered(vals)
    assert capi.png_encode_cpu(img) == ref.imencode(img)


def test_cpu_model_block_longer_than_the_window_slack():
    """A block of 16383 symbols that covers more than 32768 - 262 bytes, seven of eight symbols literals of 144 or more (nine
    bits each with the static codes): the case where zlib may have lost the block's start from its window and could not store
    it.  The encoder models no window because the stored form never wins for such a block (vsf_pe_plan_block)."""
    from vision_slam_frontend_amd import capi
    rng = np.random.default_rng(1)
    row = []
    for k in range(100):  # 6 literals of 144 .. 255, then a run of 13 (a literal and a match of 12): 8 symbols for 19 bytes
        for _ in range(6):
            v = int(rng.integers(144, 256))
            while row and v == row[-1]:
                v = 144 + (v - 143) % 112
            row.append(v)
        row += [100 + k % 40] * 13
    f = np.array([row] * 60, np.uint8)  # 60 rows of 1901 filtered bytes
    img = ref.from_filtered(f)
    data = ref.filtered(img)
    assert ref.count_symbols(data[:32506]) < 16383 < ref.count_symbols(data)  # the first block is longer than 32506 bytes
    want = ref.imencode(img)
    blocks = ref.deflate_blocks(ref.idat(want))
    assert len(blocks) >= 3 and all(n == 16383 and k != 0 for k, n in blocks[:-1]), blocks
    assert capi.png_encode_cpu(img) == want


def test_named_inputs_hold_their_features():
    kinds = lambda img: [k for k, _ in ref.deflate_blocks(ref.idat(ref.imencode(img)))]  # noqa: E731
    assert set(kinds(ref.make_input("noise", 300, 200, 1))) == {0}                     # stored
    assert set(kinds(ref.make_input("few3", 300, 200, 1))) == {2}                      # dynamic
    assert kinds(ref.make_input("ramp", 7, 5, 1)) == [1]                               # static
    assert ref.run_lengths(ref.filtered(ref.make_input("flat9", 640, 480, 1))).max() > 258
    runs = set(ref.run_lengths(ref.filtered(ref.make_input("runs", 2200, 3, 1))).tolist())
    assert set(ref.RUNS) <= runs, sorted(runs)
    assert ref.run_lengths(ref.filtered(ref.make_input("filterbyte", 64, 48, 1))).max() > 65  # through a filter byte
    for t in (16382, 16383, 16384, 16385):
        img = ref.with_symbols(t)
        blocks = ref.deflate_blocks(ref.idat(ref.imencode(img)))
        assert ref.count_symbols(ref.filtered(img)) == t == sum(n for _, n in blocks)
        assert len(blocks) == t // 16383 + 1 and all(n == 16383 for _, n in blocks[:-1]), blocks
    for t in (8191, 8192, 8193):
        assert len(ref.idat(ref.imencode(ref.with_stream_length(t)))) % 8192 == t % 8192


def test_committed_goldens_are_what_this_libpng_writes():
    cases = ref.golden_cases()
    assert len(cases) >= 10 and len(list(ref.GOLDEN.glob("*.png"))) == len(cases)
    for name, content, w, h, ch in cases:
        assert (ref.GOLDEN / (name + ".png")).read_bytes() == ref.imencode(ref.make_input(content, w, h, ch)), name


DRIVER = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import png_enc_ref as ref
L = C.CDLL(sys.argv[1])
L.vsf_png_encode_capacity.restype = C.c_size_t
L.vsf_png_encode_capacity.argtypes = [C.c_int] * 3
L.vsf_debug_png_encode_header.argtypes = [C.c_int] * 3 + [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
L.vsf_debug_png_encode_cpu.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
checked = 0
for ch in (1, 3):
    for w, h in ((1, 1), (1, 5), (7, 5), (128, 127), (128, 128), (640, 480), (65535, 65535), (65535, 1)):
        n = C.c_size_t()
        exact = np.zeros(35, np.uint8)  # a heap buffer of exactly the header's size: a byte more is an overflow
        assert L.vsf_debug_png_encode_header(w, h, ch, exact.ctypes.data, 35, C.byref(n)) == 0 and n.value == 35
        short = np.zeros(34, np.uint8)
        assert L.vsf_debug_png_encode_header(w, h, ch, short.ctypes.data, 34, C.byref(n)) == 2 and not short.any()
        assert L.vsf_png_encode_capacity(w, h, ch) > 35
        checked += 1
    for w, h in ((1, 1), (1, 5), (2, 1), (7, 5), (33, 31), (128, 127), (300, 200)):
        for c in ("flat3", "noise", "few2", "ramp"):
            img = ref.make_input(c, w, h, ch)
            want = ref.imencode(img)
            out = np.zeros(len(want), np.uint8)  # exactly the file's size
            n = C.c_size_t()
            assert L.vsf_debug_png_encode_cpu(img.ctypes.data, w, h, ch, w * ch, out.ctypes.data, len(want), C.byref(n)) == 0
            assert out.tobytes() == want, (c, w, h, ch)
            assert L.vsf_debug_png_encode_cpu(img.ctypes.data, w, h, ch, w * ch, out.ctypes.data, len(want) - 1, C.byref(n)) == 2
            checked += 1
for bad in ((0, 0, 0), (-1, 5, 1), (5, -1, 3), (1 << 30, 1 << 30, 3), (8, 8, 2)):
    n = C.c_size_t()
    buf = np.zeros(64, np.uint8)
    assert L.vsf_debug_png_encode_header(*bad, buf.ctypes.data, 64, C.byref(n)) == 1
    assert L.vsf_png_encode_capacity(*bad) == 0
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
    assert p.stdout.strip().splitlines()[-1].startswith("done checked=72"), p.stdout[-500:]
