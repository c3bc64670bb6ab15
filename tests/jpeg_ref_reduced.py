"""The system's libjpeg as cv::imdecode(IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8) drives it (tests/cpp/jpeg_ref_reduced.c, built
on demand against libjpeg.so.8): scale_num = 1, scale_denom = d, so the library runs its reduced inverse DCTs and returns
ceil(W / d) x ceil(H / d) pixels.  The yardstick of the reduced-size JPEG decode; at d = 1 it is tests/jpeg_ref.py's decode.
`available()` is False where libjpeg.so.8 itself cannot be found; a failure to compile or load the binding raises."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
_lib = None
_tried = False


def _load():
    global _lib, _tried
    if _tried:
        return _lib
    _tried = True
    # (as in jpeg_ref.py: libjpeg-turbo's SIMD routines multiply in 16 bits; the reference is the C code every libjpeg shares)
    os.environ["JSIMD_FORCENONE"] = "1"
    try:  # the one thing that may be absent: the system's library
        C.CDLL("libjpeg.so.8")
    except OSError:
        return None
    out = HERE / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libjpeg_ref_reduced.so"
    src = HERE / "cpp" / "jpeg_ref_reduced.c"
    if not so.exists() or so.stat().st_mtime < src.stat().st_mtime:
        r = subprocess.run(["gcc", "-O2", "-Wall", "-shared", "-fPIC", str(src), "-o", str(so), "-l:libjpeg.so.8"],
                           capture_output=True, text=True)
        if r.returncode != 0:  # this project's own file does not build: an error, never a skip
            raise RuntimeError("tests/cpp/jpeg_ref_reduced.c does not compile:\n" + r.stderr[-2000:])
    lib = C.CDLL(str(so))
    lib.jpeg_ref_reduced_gray.restype = C.c_int
    lib.jpeg_ref_reduced_gray.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.jpeg_ref_reduced_warnings.restype = C.c_long
    _lib = lib
    return lib


def available() -> bool:
    return _load() is not None


def reduced_size(w: int, h: int, d: int):
    return -(-w // d), -(-h // d)


def imdecode_reduced_gray(jpeg: bytes, d: int, w: int = 0, h: int = 0, max_side: int = 8192):
    """(w, h): the OUTPUT size expected, or 0, 0.  -> (status, image or None, warnings): status 0 decoded, 1 header refused,
    2 data refused, 3 another size, 4 CMYK."""
    lib = _load()
    ww, hh = C.c_int(0), C.c_int(0)
    pitch, rows = (w + 64, h) if w > 0 and h > 0 else (max_side, max_side)
    buf = np.zeros((rows, pitch), np.uint8)
    st = lib.jpeg_ref_reduced_gray(jpeg, len(jpeg), d, w, h, buf.ctypes.data, pitch, rows, C.byref(ww), C.byref(hh))
    if st != 0:
        return st, None, lib.jpeg_ref_reduced_warnings()
    return 0, buf[:hh.value, :ww.value].copy(), lib.jpeg_ref_reduced_warnings()
