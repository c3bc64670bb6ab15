"""The system's libjpeg as cv::imdecode(IMREAD_COLOR) drives it (tests/cpp/jpeg_ref_bgr.c, built on demand against
libjpeg.so.8): the reference of the colour JPEG parity tests.  `available()` is False where the library is missing."""
from __future__ import annotations

import ctypes as C
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
    # libjpeg-turbo's SIMD routines are not the C code every libjpeg shares (see jpeg_ref.py): the reference is the C code --
    # jidctint.c, jdsample.c's upsamplers and jdcolor.c's conversion.
    import os
    os.environ["JSIMD_FORCENONE"] = "1"
    out = HERE / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libjpeg_ref_bgr.so"
    src = HERE / "cpp" / "jpeg_ref_bgr.c"
    try:
        if not so.exists() or so.stat().st_mtime < src.stat().st_mtime:
            subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", str(src), "-o", str(so), "-l:libjpeg.so.8"],
                                  stderr=subprocess.DEVNULL)
        lib = C.CDLL(str(so))
    except (OSError, subprocess.CalledProcessError):
        return None
    lib.jpeg_ref_bgr_decode.restype = C.c_int
    lib.jpeg_ref_bgr_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]
    lib.jpeg_ref_bgr_warnings.restype = C.c_long
    lib.jpeg_ref_bgr_last_error_code.restype = C.c_int
    _lib = lib
    return lib


def available() -> bool:
    return _load() is not None


def last_error_code() -> int:
    """libjpeg's message code of the last fatal error (0: none)."""
    return _load().jpeg_ref_bgr_last_error_code()


def imdecode_bgr(jpeg: bytes, w: int = 0, h: int = 0, max_side: int = 4096):
    """-> (status, image (h, w, 3) in B, G, R or None, warnings): status 0 decoded, 1 header refused, 2 data refused (a fatal
    error while decoding -- a layout libjpeg has no upsampler for included), 3 another size, 4 four components."""
    lib = _load()
    ww, hh = C.c_int(0), C.c_int(0)
    pitch, rows = (3 * w + 64, h) if w > 0 and h > 0 else (3 * max_side, max_side)
    buf = np.zeros((rows, pitch), np.uint8)
    st = lib.jpeg_ref_bgr_decode(jpeg, len(jpeg), w, h, buf.ctypes.data, pitch, C.byref(ww), C.byref(hh))
    if st != 0:
        return st, None, lib.jpeg_ref_bgr_warnings()
    return 0, buf[:hh.value, :3 * ww.value].reshape(hh.value, ww.value, 3).copy(), lib.jpeg_ref_bgr_warnings()
