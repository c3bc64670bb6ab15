"""The compress side of the system's libjpeg as cv::imencode(".jpg") of OpenCV 3.2 drives it (tests/cpp/jpeg_enc_ref.c, built on
demand against libjpeg.so.8): the reference of the GPU JPEG encoder, which must write the same FILES.  Beside the binding: a
small baseline parser that counts what a file's entropy-coded segment holds (so that a fixed test input can be checked to
contain the feature it is named for) and the named inputs the tests and tools/make_jpeg_enc_golden.py share.
`available()` is False only where libjpeg.so.8 itself cannot be loaded."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
GOLDEN = HERE / "golden" / "jpeg_enc"
_lib = None
_tried = False


def _load():
    global _lib, _tried
    if _tried:
        return _lib
    _tried = True
    os.environ["JSIMD_FORCENONE"] = "1"  # the reference is the C code every libjpeg shares (as tests/jpeg_ref.py)
    out = HERE / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libjpeg_enc_ref.so"
    src = HERE / "cpp" / "jpeg_enc_ref.c"
    try:
        C.CDLL("libjpeg.so.8")
    except OSError:
        return None  # the one reason to be unavailable: the library itself cannot be loaded
    if not so.exists() or so.stat().st_mtime < src.stat().st_mtime:  # (a compile error in the binding is an error, not a skip)
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", str(src), "-o", str(so), "-l:libjpeg.so.8"])
    lib = C.CDLL(str(so))
    lib.jpeg_enc_ref.restype = C.c_long
    lib.jpeg_enc_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]
    _lib = lib
    return lib


def available() -> bool:
    return _load() is not None


def imencode(img: np.ndarray, quality: int = 95) -> bytes:
    """cv::imencode(".jpg", img, {IMWRITE_JPEG_QUALITY, quality}): img is (h, w) gray or (h, w, 3) BGR, uint8."""
    lib = _load()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    ch = 1 if img.ndim == 2 else img.shape[2]
    h, w = img.shape[:2]
    cap = 4096 + 8 * w * h * ch
    out = np.zeros(cap, np.uint8)
    n = lib.jpeg_enc_ref(img.ctypes.data, w, h, ch, w * ch, quality, out.ctypes.data, cap)
    if n <= 0 or n > cap:
        raise RuntimeError("libjpeg refused to encode (%d)" % n)
    return out[:n].tobytes()


# ---- a small parser of what libjpeg wrote -----------------------------------------------------------------------------------

def header_length(jpeg: bytes) -> int:
    """Bytes from SOI up to and including the SOS header (the entropy-coded segment starts there)."""
    assert jpeg[:2] == b"\xff\xd8"
    p = 2
    while True:
        assert jpeg[p] == 0xFF
        m, n = jpeg[p + 1], (jpeg[p + 2] << 8) | jpeg[p + 3]
        p += 2 + n
        if m == 0xDA:
            return p


def scan_stats(jpeg: bytes) -> dict:
    """Decodes the symbols of a baseline file's one scan -> {stuffed (FF 00 pairs), zrl (F0 symbols), eob, max_size (largest
    size category of any coefficient), blocks, max_zrl_run (most ZRLs in a row)}."""
    p, huff, comps, sof = 2, {}, [], None
    while True:
        m, n = jpeg[p + 1], (jpeg[p + 2] << 8) | jpeg[p + 3]
        seg = jpeg[p + 4:p + 2 + n]
        if m == 0xC4:
            q = 0
            while q < len(seg):
                tc_th, bits = seg[q], seg[q + 1:q + 17]
                vals = seg[q + 17:q + 17 + sum(bits)]
                q += 17 + sum(bits)
                table, code, k = {}, 0, 0
                for ln in range(1, 17):
                    for _ in range(bits[ln - 1]):
                        table[(ln, code)] = vals[k]
                        code += 1
                        k += 1
                    code <<= 1
                huff[tc_th] = table
        elif m == 0xC0:
            sof = seg
            hh, ww, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15) for i in range(nc)]
        elif m == 0xDA:
            sel = {seg[1 + 2 * i]: (seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(seg[0])}
            p += 2 + n
            break
        p += 2 + n
    assert sof is not None and jpeg[-2:] == b"\xff\xd9"
    raw = jpeg[p:-2]
    stuffed = raw.count(b"\xff\x00")
    data = raw.replace(b"\xff\x00", b"\xff")
    bits = np.unpackbits(np.frombuffer(data, np.uint8))
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    if len(comps) == 1:
        n_mcu, per_mcu = ((ww + 7) // 8) * ((hh + 7) // 8), [comps[0][0]]
    else:
        n_mcu = ((ww + 8 * hmax - 1) // (8 * hmax)) * ((hh + 8 * vmax - 1) // (8 * vmax))
        per_mcu = [c[0] for c in comps for _ in range(c[1] * c[2])]
    pos = 0

    def symbol(table):
        nonlocal pos
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | int(bits[pos])
            pos += 1
            if (ln, code) in table:
                return table[(ln, code)]
        raise AssertionError("bad code")

    st = dict(stuffed=stuffed, zrl=0, eob=0, max_size=0, blocks=0, max_zrl_run=0)
    for _ in range(n_mcu):
        for cid in per_mcu:
            td, ta = sel[cid]
            s = symbol(huff[td])
            st["max_size"] = max(st["max_size"], s)
            pos += s
            k, run = 1, 0
            while k < 64:
                rs = symbol(huff[0x10 | ta])
                r, s = rs >> 4, rs & 15
                if s == 0:
                    if r == 15:
                        st["zrl"] += 1
                        run += 1
                        st["max_zrl_run"] = max(st["max_zrl_run"], run)
                        k += 16
                        continue
                    st["eob"] += 1
                    break
                run = 0
                k += r
                st["max_size"] = max(st["max_size"], s)
                pos += s
                k += 1
            st["blocks"] += 1
    assert len(bits) - pos < 8 and bits[pos:].all(), "the scan does not end in 1-bit padding"
    return st


# ---- the named inputs ---------------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 9), (33, 31), (64, 48)]  # (width, height)
QUALITIES = [1, 50, 95, 100]
CONTENTS_GRAY = ["flat0", "flat128", "flat255", "ramp", "noise", "checker", "zz63"]
CONTENTS_BGR = CONTENTS_GRAY + ["stripes"]


def make_input(content: str, w: int, h: int, channels: int, seed: int = 0) -> np.ndarray:
    """The (h, w) / (h, w, 3) uint8 test image called `content`."""
    y, x = np.mgrid[0:h, 0:w]
    if content.startswith("flat"):
        g = np.full((h, w), int(content[4:]), np.uint8)
    elif content == "ramp":  # horizontal
        g = (x * 255 // max(w - 1, 1)).astype(np.uint8)
    elif content == "noise":
        rng = np.random.default_rng(1000 + seed + 7 * w + 13 * h + channels)
        return rng.integers(0, 256, (h, w) if channels == 1 else (h, w, 3), dtype=np.uint8)
    elif content == "checker":  # 128 +- 127 in a 1-pixel checkerboard: its energy sits in the highest frequencies
        g = np.where((x + y) & 1, 1, 255).astype(np.uint8)
    elif content == "zz63":  # the basis function of coefficient (7, 7) alone: one non-zero coefficient at zig-zag 63
        c = np.cos((2 * (np.arange(max(w, h)) % 8) + 1) * 7 * np.pi / 16)
        g = np.clip(np.rint(128 + 127 * c[y] * c[x]), 0, 255).astype(np.uint8)
    elif content == "stripes":  # saturated primaries in 1-pixel stripes: vertical in the upper half, horizontal below
        assert channels == 3
        k = np.where(y < (h + 1) // 2, x, y) % 3
        return np.stack([(k == 0) * 255, (k == 1) * 255, (k == 2) * 255], -1).astype(np.uint8)
    else:
        raise ValueError(content)
    if channels == 1:
        return g
    if content == "noise":
        raise AssertionError
    if content == "ramp":  # the three channels ramp at different rates
        return np.stack([g, 255 - g, (x * 3 % 256).astype(np.uint8)], -1)
    return np.stack([g, g, g], -1)


def golden_cases():
    """(file name, content, w, h, channels, quality) of the committed files of tests/golden/jpeg_enc."""
    return [("gray_1x1_flat128_q95", "flat128", 1, 1, 1, 95), ("gray_17x9_ramp_q50", "ramp", 17, 9, 1, 50),
            ("gray_33x31_noise_q100", "noise", 33, 31, 1, 100), ("gray_16x16_checker_q100", "checker", 16, 16, 1, 100),
            ("gray_64x48_zz63_q50", "zz63", 64, 48, 1, 50), ("gray_7x5_noise_q1", "noise", 7, 5, 1, 1),
            ("bgr_1x1_flat255_q95", "flat255", 1, 1, 3, 95), ("bgr_17x9_stripes_q95", "stripes", 17, 9, 3, 95),
            ("bgr_33x31_noise_q100", "noise", 33, 31, 3, 100), ("bgr_16x16_checker_q100", "checker", 16, 16, 3, 100),
            ("bgr_64x48_ramp_q50", "ramp", 64, 48, 3, 50), ("bgr_7x5_stripes_q1", "stripes", 7, 5, 3, 1),
            ("bgr_64x48_zz63_q50", "zz63", 64, 48, 3, 50)]
