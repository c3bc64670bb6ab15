"""The write side of the system's libpng as cv::imencode(".png") of OpenCV 3.2 drives it without parameters
(tests/cpp/png_enc_ref.c, built on demand against libpng16.so.16): the reference of the GPU PNG encoder, which must write the same
FILES.  Beside the binding: the zlib model of such a file (Sub-filtered rows, deflate level 1 / memLevel 8 / Z_RLE, IDAT chunks of
8192 bytes), which pins the binding itself; a symbol counter for deflate_rle's parse and a reader of the blocks of a deflate
stream, so that a fixed test input can be checked to hold the feature it is named for; and the named inputs the tests and
tools/make_png_enc_golden.py share.  `available()` is False only where libpng16.so.16 itself cannot be loaded."""
from __future__ import annotations

import ctypes as C
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
GOLDEN = HERE / "golden" / "png_enc"
_lib = None
_tried = False


def _load():
    global _lib, _tried
    if _tried:
        return _lib
    _tried = True
    out = HERE / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    so = out / "libpng_enc_ref.so"
    src = HERE / "cpp" / "png_enc_ref.c"
    try:
        C.CDLL("libpng16.so.16")
    except OSError:
        return None  # the one reason to be unavailable: the library itself cannot be loaded
    if not so.exists() or so.stat().st_mtime < src.stat().st_mtime:  # (a compile error in the binding is an error, not a skip)
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", str(src), "-o", str(so), "-l:libpng16.so.16"])
    lib = C.CDLL(str(so))
    lib.png_enc_ref.restype = C.c_long
    lib.png_enc_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t]
    _lib = lib
    return lib


def available() -> bool:
    return _load() is not None


def imencode(img: np.ndarray) -> bytes:
    """cv::imencode(".png", img): img is (h, w) gray or (h, w, 3) BGR, uint8."""
    lib = _load()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    ch = 1 if img.ndim == 2 else img.shape[2]
    h, w = img.shape[:2]
    cap = 4096 + 2 * w * h * ch
    out = np.zeros(cap, np.uint8)
    n = lib.png_enc_ref(img.ctypes.data, w, h, ch, w * ch, out.ctypes.data, cap)
    if n <= 0 or n > cap:
        raise RuntimeError("libpng refused to encode (%d)" % n)
    return out[:n].tobytes()


# ---- the zlib model ----------------------------------------------------------------------------------------------------------

def filtered(img: np.ndarray) -> bytes:
    """The rows as libpng hands them to zlib: R G B order, Sub (type 1) -- type 0 where the image is one pixel wide."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    px = img.reshape(h, w, -1)[:, :, ::-1].astype(np.int16)
    sub = px.copy()
    sub[:, 1:] -= px[:, :-1]
    rows = np.empty((h, 1 + w * px.shape[2]), np.uint8)
    rows[:, 0] = 0 if w == 1 else 1
    rows[:, 1:] = (sub & 255).astype(np.uint8).reshape(h, -1)
    return rows.tobytes()


def stream_header(n_filtered: int) -> bytes:
    """The two bytes in front of the deflate stream.  libpng 1.6 shrinks the window it asks zlib for while the filtered image
    plus 262 bytes fits half of it (png_deflate_claim), and rewrites CINFO once more when the first IDAT leaves (optimize_cmf);
    both only for images of at most 16384 filtered bytes.  Level 1: FLEVEL 0."""
    cinfo = 7
    if n_filtered <= 16384:
        half = 1 << 14
        while n_filtered + 262 <= half:
            half >>= 1
            cinfo -= 1
        half = 1 << (cinfo + 7)
        if n_filtered <= half:
            while True:
                half >>= 1
                cinfo -= 1
                if not (cinfo > 0 and n_filtered <= half):
                    break
    cmf = (cinfo << 4) | 8
    return bytes([cmf, 31 - (cmf << 8) % 31])


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def zlib_stream(img: np.ndarray) -> bytes:
    raw = filtered(img)
    co = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    z = co.compress(raw) + co.flush()
    assert z[:2] == b"\x78\x01"
    return stream_header(len(raw)) + z[2:]


def model(img: np.ndarray) -> bytes:
    """The file as the zlib model predicts it."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    z = zlib_stream(img)
    out = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if ch == 1 else 2, 0, 0, 0))
    for p in range(0, len(z), 8192):
        out += _chunk(b"IDAT", z[p:p + 8192])
    return out + _chunk(b"IEND", b"")


# ---- what a file holds -------------------------------------------------------------------------------------------------------

def idat(png: bytes) -> bytes:
    """The zlib stream of a file (its IDAT chunks joined)."""
    p, out = 8, b""
    while p < len(png):
        n, kind = struct.unpack(">I4s", png[p:p + 8])
        if kind == b"IDAT":
            out += png[p + 8:p + 8 + n]
        p += 12 + n
    return out


def idat_sizes(png: bytes) -> list:
    p, out = 8, []
    while p < len(png):
        n, kind = struct.unpack(">I4s", png[p:p + 8])
        if kind == b"IDAT":
            out.append(n)
        p += 12 + n
    return out


def run_lengths(data: bytes) -> np.ndarray:
    a = np.frombuffer(data, np.uint8)
    starts = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
    return np.diff(np.concatenate((starts, [len(a)])))


def count_symbols(data: bytes) -> int:
    """Literals and matches of deflate_rle's greedy parse: per run one literal, then matches of min(258, rest) while at least 3
    bytes remain, then literals."""
    rest = run_lengths(data).astype(np.int64) - 1
    tail = rest % 258
    return int((1 + rest // 258 + np.where(tail >= 3, 1, tail)).sum())


_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_EXTRA = [0, 0, 0, 0] + [b for b in range(1, 14) for _ in (0, 1)]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def deflate_blocks(z: bytes) -> list:
    """(type, symbols) of every block of a zlib stream: type 0 stored, 1 static, 2 dynamic; symbols: literals + matches (a stored
    block's count is its bytes)."""
    bits = np.unpackbits(np.frombuffer(z[2:], np.uint8), bitorder="little")
    pos = 0

    def take(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= int(bits[pos + i]) << i
        pos += n
        return v

    def table(lengths):
        count = [0] * 16
        for ln in lengths:
            count[ln] += 1
        count[0] = 0
        code, nxt = 0, [0] * 16
        for ln in range(1, 16):
            code = (code + count[ln - 1]) << 1
            nxt[ln] = code
        t = {}
        for sym, ln in enumerate(lengths):
            if ln:
                t[(ln, nxt[ln])] = sym
                nxt[ln] += 1
        return t

    def symbol(t):
        nonlocal pos
        code = 0
        for ln in range(1, 16):
            code = (code << 1) | int(bits[pos])
            pos += 1
            if (ln, code) in t:
                return t[(ln, code)]
        raise AssertionError("bad code")

    static_l = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
    static_d = table([5] * 30)
    out = []
    while True:
        last, kind = take(1), take(2)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = take(16)
            assert take(16) == n ^ 0xFFFF
            pos += 8 * n
            out.append((0, n))
        else:
            if kind == 1:
                tl, td = static_l, static_d
            else:
                nl, nd, nc = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for i in range(nc):
                    cl[_CL_ORDER[i]] = take(3)
                tc, lens = table(cl), []
                while len(lens) < nl + nd:
                    s = symbol(tc)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + take(2))
                    elif s == 17:
                        lens += [0] * (3 + take(3))
                    else:
                        lens += [0] * (11 + take(7))
                tl, td = table(lens[:nl]), table(lens[nl:])
            n = 0
            while True:
                s = symbol(tl)
                if s == 256:
                    break
                n += 1
                if s > 256:
                    pos += _LEN_EXTRA[s - 257]
                    d = symbol(td)  # (reads bits: not inside the += below)
                    pos += _DIST_EXTRA[d]
            out.append((kind, n))
        if last:
            return out


# ---- the named inputs --------------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (1, 5), (2, 1), (3, 3), (7, 5), (33, 31), (64, 48), (128, 127), (128, 128), (300, 200), (640, 480)]
RUNS = [1, 2, 3, 4, 258, 259, 260, 261, 262, 517]


def _shape(w, h, ch):
    return (h, w) if ch == 1 else (h, w, 3)


def from_filtered(rows: np.ndarray, channels: int = 1) -> np.ndarray:
    """The gray image whose Sub-filtered rows are `rows` ((h, w) uint8): the running sum along each row."""
    assert channels == 1
    return (np.cumsum(rows.astype(np.int64), axis=1) & 255).astype(np.uint8)


def make_input(content: str, w: int, h: int, channels: int, seed: int = 0) -> np.ndarray:
    """The (h, w) / (h, w, 3) uint8 test image called `content`."""
    rng = np.random.default_rng(2000 + seed + 7 * w + 13 * h + channels)
    y, x = np.mgrid[0:h, 0:w]
    if content.startswith("flat"):
        return np.full(_shape(w, h, channels), int(content[4:]), np.uint8)
    if content == "noise":  # incompressible: stored blocks
        return rng.integers(0, 256, _shape(w, h, channels), dtype=np.uint8)
    if content.startswith("few"):  # noise over 2 - 4 values of the FILTERED stream: dynamic blocks with short codes
        k = int(content[3:])
        d = rng.integers(0, k, (h, w * channels)).astype(np.int64) * 3
        if channels == 1:
            return (np.cumsum(d, axis=1) & 255).astype(np.uint8)
        return (np.cumsum(d.reshape(h, w, 3), axis=1) & 255).astype(np.uint8)
    if content == "ramp":  # every byte differs from the one before: literals only, in a tiny image a static block
        g = ((x * 37 + y * 11) & 255).astype(np.uint8)
        return g if channels == 1 else np.stack([g, g + 85, g + 170], -1).astype(np.uint8)
    if content == "channels":  # three distinct channels: B G R in memory, R G B in the file
        assert channels == 3
        return np.stack([(x * 3 + y) & 255, 255 - ((x + y * 5) & 255), (x * y) & 255], -1).astype(np.uint8)
    if content == "runs":  # every row of the filtered stream holds runs of exactly RUNS bytes, each between two other values
        assert channels == 1 and w >= sum(RUNS) + 2 * len(RUNS)
        row, v = [], 10
        for n in RUNS:
            row += [v] * n + [v + 100]  # (a single other byte behind each run)
            v += 3
        row += [(200 + (i & 1)) for i in range(w - len(row))]
        f = np.array([row[y % 7:] + row[:y % 7] for y in range(h)], np.uint8)  # (rotated: the runs meet the tiles elsewhere)
        return from_filtered(f)
    if content == "filterbyte":  # rows end and begin with 1s: the runs of the filtered stream run THROUGH the filter byte
        assert channels == 1
        f = np.ones((h, w), np.uint8)
        f[::3, w // 2] = 9
        return from_filtered(f)
    raise ValueError(content)


def with_symbols(target: int, w: int = 127) -> np.ndarray:
    """A gray image whose filtered stream parses into exactly `target` symbols.  Every byte of a row that alternates between 2
    and 3 behind its filter byte is a literal; a run of L >= 4 equal bytes at a row's end is two symbols and so takes L - 2 away."""
    rows = -(-target // (w + 1)) + 1
    f = np.empty((rows, w), np.uint8)
    f[:] = np.where(np.arange(w) & 1, 3, 2)
    k = rows * (w + 1) - target
    r = rows - 1
    while k > 0:
        red = min(k, w - 2)
        if k - red == 1:
            red -= 1
        f[r, w - (red + 2):] = 7
        k -= red
        r -= 1
    img = from_filtered(f)
    assert count_symbols(filtered(img)) == target
    return img


def with_stream_length(residue: int) -> np.ndarray:
    """A gray noise image whose zlib stream is `residue` bytes long modulo the IDAT size of 8192.  Noise of n filtered bytes is
    n // 16383 + 1 stored blocks of 5 bytes each around it, behind 2 bytes and in front of 4; the search over shapes and seeds
    checks that against zlib itself."""
    for n in range(8000, 60000):
        if (2 + 5 * (n // 16383 + 1) + n + 4) % 8192 != residue % 8192:
            continue
        for rowbytes in range(3000, 150, -1):  # (long rows: the filter bytes do not tip the block to a dynamic one)
            if n % rowbytes == 0:
                for seed in range(4):
                    img = np.random.default_rng(seed).integers(0, 256, (n // rowbytes, rowbytes - 1), dtype=np.uint8)
                    if len(zlib_stream(img)) % 8192 == residue % 8192:
                        return img
    raise AssertionError("no image with a stream of %d bytes mod 8192" % residue)


def golden_cases():
    """(file name, content, w, h, channels) of the committed files of tests/golden/png_enc."""
    return [("gray_1x1_flat128", "flat128", 1, 1, 1), ("gray_1x5_noise", "noise", 1, 5, 1), ("gray_7x5_ramp", "ramp", 7, 5, 1),
            ("gray_33x31_noise", "noise", 33, 31, 1), ("gray_64x48_few3", "few3", 64, 48, 1),
            ("gray_128x127_flat7", "flat7", 128, 127, 1), ("gray_2200x3_runs", "runs", 2200, 3, 1),
            ("gray_64x48_filterbyte", "filterbyte", 64, 48, 1), ("bgr_1x1_flat255", "flat255", 1, 1, 3),
            ("bgr_33x31_channels", "channels", 33, 31, 3), ("bgr_64x48_few4", "few4", 64, 48, 3),
            ("bgr_7x5_noise", "noise", 7, 5, 3)]
