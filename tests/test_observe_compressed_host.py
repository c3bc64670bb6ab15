"""The host side of vsf_observe_submit_compressed that needs no device (csrc/vsf_ingest_host.cc): the sizes of the pinned
ring the compressed files wait in, and what a submit does with ONE payload before it books anything
(vsf_observe_probe_compressed: the format by the first bytes, the byte cap -> VSF_ERR_CAPACITY, then the decoder's own host
checks).  The payloads are UNTRUSTED (slam_frontend_main.cc:98-100 hands cv::imdecode whatever the topic carried), so the same
translation unit is part of the sanitizer build (`make asan`, as tests/test_jpeg_host_asan.py shows) and the probe runs there
over the fixtures and the damaged-file generator tests/jpeg_mutate.py."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vision_slam_frontend_amd" / "csrc"
LIB = ROOT / "vision_slam_frontend_amd" / "libvsf_jpeg_host_asan.so"
GOLD = Path(__file__).resolve().parent / "golden"
OK, INVALID, CAPACITY, UNSUPPORTED = 0, 1, 2, 4


def _probe(L, data: bytes, w: int, h: int, cap: int, serial: int = 0):
    kind = C.c_int(-1)
    buf = np.frombuffer(bytes(data), np.uint8)
    st = L.vsf_observe_probe_compressed(buf.ctypes.data_as(C.c_void_p), len(buf), w, h, cap, serial, C.byref(kind))
    return st, kind.value


def test_ring_sizing():
    from vision_slam_frontend_amd import capi
    L = capi.lib()
    # the default cap: a lossless file of a noisy image is a little larger than the image
    assert L.vsf_observe_default_compressed_cap(640, 480) == 640 * 480 + 65536
    assert L.vsf_observe_default_compressed_cap(0, 480) == 0
    # a slot is the cap rounded up to 64 bytes; the ring is depth x 2 slots
    for cap in (1, 63, 64, 65, 100000, 640 * 480 + 65536, 1 << 30):
        slot = L.vsf_observe_compressed_slot_bytes(cap)
        assert slot >= cap and slot % 64 == 0 and slot - cap < 64
        for depth in (1, 4, 256, 1024):
            assert L.vsf_observe_compressed_ring_bytes(depth, cap) == depth * 2 * slot
    assert L.vsf_observe_compressed_slot_bytes(0) == 0 and L.vsf_observe_compressed_slot_bytes((1 << 30) + 1) == 0
    for depth, cap in ((0, 1000), (-1, 1000), (1025, 1000), (4, 0), (4, (1 << 30) + 1)):
        assert L.vsf_observe_compressed_ring_bytes(depth, cap) == 0, (depth, cap)
    # the queue at the benched shape (depth 256, 640x480) pins 182 MB for compressed frames, 4 MB at a 8 KB cap
    assert L.vsf_observe_compressed_ring_bytes(256, 640 * 480 + 65536) == 256 * 2 * 372736
    assert L.vsf_observe_compressed_ring_bytes(256, 8192) == 4 << 20


def test_probe_tells_formats_and_enforces_the_cap():
    from vision_slam_frontend_amd import capi
    L = capi.lib()
    expected = np.load(GOLD / "jpeg" / "expected_gray.npz")
    jpg = (GOLD / "jpeg" / "gray_320x240_q80.jpg").read_bytes()
    prog = (GOLD / "jpeg" / "prog_gray_320x240_q85.jpg").read_bytes()
    png = (GOLD / "png" / "pil_photo_level6.png").read_bytes()
    ph, pw = np.load(GOLD / "png" / "expected_gray.npz")["pil_photo_level6"].shape
    assert expected["gray_320x240_q80"].shape == (240, 320)
    assert _probe(L, jpg, 320, 240, len(jpg)) == (OK, 1)
    assert _probe(L, prog, 320, 240, 1 << 20) == (OK, 1)
    assert _probe(L, png, pw, ph, len(png)) == (OK, 2)
    # one byte above the cap: VSF_ERR_CAPACITY, whatever the file is like otherwise -- and before it is parsed
    assert _probe(L, jpg, 320, 240, len(jpg) - 1) == (CAPACITY, 0)
    assert _probe(L, png, pw, ph, len(png) - 1) == (CAPACITY, 0)
    assert _probe(L, jpg[:200] + bytes(5000), 320, 240, 1000) == (CAPACITY, 0)
    # the decoders' own refusals come through unchanged
    assert _probe(L, jpg, 321, 240, 1 << 20) == (INVALID, 0)          # another size
    assert _probe(L, jpg[:100], 320, 240, 1 << 20) == (INVALID, 0)    # cut inside the headers
    assert _probe(L, png[:30], pw, ph, 1 << 20) == (INVALID, 0)
    assert _probe(L, b"BM" + bytes(100), 320, 240, 1 << 20) == (UNSUPPORTED, 0)
    assert _probe(L, b"", 320, 240, 1 << 20) == (UNSUPPORTED, 0)
    # ... and the size a header states (what sizes a Frontend's context from its first compressed frame)
    w, h = C.c_int(), C.c_int()
    for data, want in ((jpg, (320, 240)), (prog, (320, 240)), (png, (pw, ph))):
        buf = np.frombuffer(data, np.uint8)
        assert L.vsf_compressed_image_size(buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(w), C.byref(h)) == OK
        assert (w.value, h.value) == want
    buf = np.frombuffer(jpg[:20], np.uint8)
    assert L.vsf_compressed_image_size(buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(w), C.byref(h)) == INVALID


DRIVER = r'''
import ctypes as C, sys
from pathlib import Path
import numpy as np
sys.path.insert(0, sys.argv[3])
from jpeg_mutate import mutate
lib = C.CDLL(sys.argv[1])
lib.vsf_observe_probe_compressed.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_int)]
lib.vsf_compressed_image_size.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
gold = Path(sys.argv[2])
jpeg_shapes = np.load(gold / "jpeg" / "expected_gray.npz")
png_shapes = np.load(gold / "png" / "expected_gray.npz")
files = [(p.read_bytes(), jpeg_shapes[p.stem].shape) for p in sorted((gold / "jpeg").glob("*.jpg"))]
files += [(p.read_bytes(), png_shapes[p.stem].shape) for p in sorted((gold / "png").glob("*.png")) if p.stem in png_shapes.files]

def probe(data, w, h, cap, serial=0):
    # (an exact-size heap copy: the sanitizer sees a read one byte past the payload)
    buf = C.create_string_buffer(data, len(data)) if data else C.create_string_buffer(1)
    kind, ww, hh = C.c_int(), C.c_int(), C.c_int()
    st = lib.vsf_observe_probe_compressed(C.cast(buf, C.c_char_p), len(data), w, h, cap, serial, C.byref(kind))
    s2 = lib.vsf_compressed_image_size(C.cast(buf, C.c_char_p), len(data), C.byref(ww), C.byref(hh))
    assert s2 in (0, 1, 4)
    return st, kind.value

ok = bad = 0
for data, (h, w) in files:
    st, kind = probe(data, w, h, len(data))
    assert st in (0, 4) and (st != 0 or kind in (1, 2)), (st, kind)  # (a few fixtures are kinds the decoders do not take)
    assert probe(data, w, h, len(data) - 1)[0] == 2
rng = np.random.Generator(np.random.PCG64(20261016))
for it in range(2500):
    data, (h, w) = files[int(rng.integers(len(files)))]
    m = mutate(data, rng)
    st, kind = probe(m, w, h, 1 << 22, int(rng.integers(2)))
    assert st in (0, 1, 4), st   # VSF_OK, VSF_ERR_INVALID_ARG, VSF_ERR_UNSUPPORTED: never anything else, never a crash
    ok += st == 0
    bad += st != 0
    cut = m[:int(rng.integers(0, len(m) + 1))]
    assert probe(cut, w, h, 1 << 22)[0] in (0, 1, 4)
for junk in (b"", b"\xff", b"\xff\xd8\xff", b"\x89PNG\r\n\x1a\n", b"\x89PNG\r\n\x1a\n" + bytes(16), bytes(64)):
    assert probe(junk, 8, 8, 1 << 20)[0] in (1, 4), junk[:8]
print("done ok=%d refused=%d" % (ok, bad))
'''


def test_submit_side_parser_under_asan_and_ubsan(tmp_path):
    asan_rt = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    ubsan_rt = subprocess.run(["gcc", "-print-file-name=libubsan.so"], capture_output=True, text=True).stdout.strip()
    if not (asan_rt and Path(asan_rt).exists() and ubsan_rt and Path(ubsan_rt).exists()):
        pytest.skip("no sanitizer runtime in this toolchain")
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "asan"], capture_output=True, text=True)
    assert r.returncode == 0 and LIB.exists(), r.stderr[-2000:]
    script = tmp_path / "drive.py"
    script.write_text(DRIVER)
    env = dict(os.environ, LD_PRELOAD="%s %s" % (asan_rt, ubsan_rt),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([sys.executable, str(script), str(LIB), str(GOLD), str(Path(__file__).resolve().parent)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-4000:])
    last = p.stdout.strip().splitlines()[-1]
    assert last.startswith("done"), p.stdout[-500:]
    ok = int(last.split("ok=")[1].split()[0])
    refused = int(last.split("refused=")[1].split()[0])
    assert ok > 300 and refused > 100  # the damage reached both the accepting and the refusing paths
