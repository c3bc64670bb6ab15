"""libjpeg's colour-space decision (jdapimin.c default_decompress_parms) as the host parser makes it for a colour read
(csrc/vsf_jpeg_host.cc), on crafted headers: a JFIF marker, the Adobe marker with transform 0 / 1 / 2, the component ids
'R' 'G' 'B', 1 2 3 and others, and their combinations.  The parser runs in a stand-alone program (tests/cpp/
test_jpeg_colourspace.cc, linked with the host sources), once plainly and once under AddressSanitizer + UBSan with a few
thousand mutated headers on top; nothing is preloaded and nothing is loaded into Python.  Each verdict is held against the
system's libjpeg: a file the parser takes as YCbCr must decode to the pixels of the unmarked file (ids 1 2 3: YCbCr), a file
it refuses as RGB (VSF_ERR_UNSUPPORTED -- followed or refused, never guessed) must decode to other pixels there."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import imdecode_bgr_cases as cases_bgr
import jpeg_craft as jc
import jpeg_ref_bgr

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vision_slam_frontend_amd" / "csrc"
SRCS = [str(ROOT / "tests" / "cpp" / "test_jpeg_colourspace.cc")] + \
       [str(CSRC / n) for n in ("vsf_jpeg_host.cc", "vsf_png_host.cc", "vsf_ingest_host.cc", "vsf_jpeg_enc_host.cc",
                                "vsf_png_enc_host.cc", "vsf_jpeg_host_check.cc")]
VSF_OK, VSF_ERR_INVALID_ARG, VSF_ERR_UNSUPPORTED = 0, 1, 4   # include/vsf.h
W, H = 24, 16


def seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


JFIF = seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
JFIF_SHORT = seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00")      # 13 data bytes: not a JFIF marker to libjpeg
JFXX = seg(0xE0, b"JFXX\x00\x10" + bytes(8))


def adobe(transform, n=12):
    return seg(0xEE, (b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([transform]))[:n])


def with_ids(data, ids):
    """The file with its component ids (1, 2, 3 as jpeg_craft writes them) replaced in the frame and the scan header."""
    b = bytearray(data)
    pos = 2
    while pos < len(b):
        m, ln = b[pos + 1], (b[pos + 2] << 8) | b[pos + 3]
        if m == 0xC0:
            for c in range(3):
                assert b[pos + 10 + 3 * c] == c + 1
                b[pos + 10 + 3 * c] = ids[c]
        if m == 0xDA:
            for c in range(3):
                assert b[pos + 5 + 2 * c] == c + 1
                b[pos + 5 + 2 * c] = ids[c]
            return bytes(b)
        pos += 2 + ln
    raise AssertionError("no scan")


def headers():
    """-> [(name, bytes, status of the colour read)]"""
    base = cases_bgr.upsampler_file(np.random.default_rng(5), W, H, cases_bgr.LAYOUTS["420"], 0)
    ins = lambda *segs: base[:2] + b"".join(segs) + base[2:]
    rgb, other = (ord("R"), ord("G"), ord("B")), (0, 1, 2)
    return [
        ("ids_1_2_3", base, VSF_OK),
        ("jfif", ins(JFIF), VSF_OK),
        ("adobe_0", ins(adobe(0)), VSF_ERR_UNSUPPORTED),
        ("adobe_1", ins(adobe(1)), VSF_OK),
        ("adobe_2", ins(adobe(2)), VSF_OK),                       # (libjpeg warns and assumes YCbCr)
        ("adobe_0_too_short", ins(adobe(0, 11)), VSF_OK),         # (not an Adobe marker to libjpeg: 11 data bytes)
        ("jfif_and_adobe_0", ins(JFIF, adobe(0)), VSF_OK),        # (JFIF decides)
        ("adobe_0_and_jfif", ins(adobe(0), JFIF), VSF_OK),
        ("jfif_short_and_adobe_0", ins(JFIF_SHORT, adobe(0)), VSF_ERR_UNSUPPORTED),
        ("jfxx_only_ids_rgb", with_ids(ins(JFXX), rgb), VSF_ERR_UNSUPPORTED),
        ("ids_rgb", with_ids(base, rgb), VSF_ERR_UNSUPPORTED),
        ("ids_rgb_jfif", with_ids(ins(JFIF), rgb), VSF_OK),
        ("ids_rgb_adobe_1", with_ids(ins(adobe(1)), rgb), VSF_OK),
        ("ids_0_1_2", with_ids(base, other), VSF_OK),             # (ids libjpeg does not know: YCbCr, with a trace message)
        ("ids_rgb_lower_case", with_ids(base, (ord("r"), ord("g"), ord("b"))), VSF_OK),
    ]


@pytest.mark.parametrize("flags,rounds", [(["-O2"], 50), (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], 300)],
                         ids=["plain", "asan_ubsan"])
def test_colour_space_decision(tmp_path, flags, rounds):
    exe = tmp_path / "test_jpeg_colourspace"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        "-o", str(exe), *SRCS, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = headers()
    # beside them: layouts and processes, for the refusals a colour read adds to a gray one
    extra = [(c[0], c[1], c[2], c[3], c[4], c[5]) for c in jc.sampling_cases() if (c[2], c[3]) == (75, 61)]
    lines = []
    for i, (name, data, _) in enumerate(cases):
        (tmp_path / ("h%02d.jpg" % i)).write_bytes(data)
        lines.append("%s %d %d" % (tmp_path / ("h%02d.jpg" % i), W, H))
    for i, (name, data, w, h, factors, process) in enumerate(extra):
        (tmp_path / ("s%03d.jpg" % i)).write_bytes(data)
        lines.append("%s %d %d" % (tmp_path / ("s%03d.jpg" % i), w, h))
    (tmp_path / "manifest.txt").write_text("\n".join(lines) + "\n")
    p = subprocess.run([str(exe), str(tmp_path / "manifest.txt"), str(rounds)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    out = p.stdout.splitlines()
    assert out[-1].startswith("ok jpeg colourspace: %d files" % len(lines)), out[-1]
    got = {int(f[1]): tuple(int(t) for t in f[2:]) for f in (l.split() for l in out[:-1])}
    assert jpeg_ref_bgr.available()
    _, plain, warn = jpeg_ref_bgr.imdecode_bgr(cases[0][1], W, H)
    assert warn == 0
    for i, (name, data, want) in enumerate(cases):
        colour, gray, bytes_colour, bytes_gray = got[i][:4]
        assert colour == want, name
        assert gray == VSF_OK, name                       # (a gray read takes the first component whatever it is called)
        st, ref, _ = jpeg_ref_bgr.imdecode_bgr(data, W, H)
        assert st == 0, name
        assert np.array_equal(ref, plain) == (want == VSF_OK), "%s: libjpeg reads it %s" % (name, "as RGB" if want == VSF_OK else "as YCbCr")
        if want == VSF_OK:
            assert bytes_colour >= bytes_gray + 256, name   # (the two chroma quantisation tables travel with a colour read)
    for i, (name, data, w, h, factors, process) in enumerate(extra):
        colour, gray, _, _, n_par, n_prog = got[len(cases) + i]
        assert gray == VSF_OK, name
        st, _, warn = jpeg_ref_bgr.imdecode_bgr(data, w, h)
        if st == 0:
            assert colour == VSF_OK, name
            # the decoder a colour read takes: one-scan files the parallel one, files in several scans the scan-list one
            assert (n_par, n_prog) == ((1, 0) if process in ("base", "base_rst") else (0, 1)), name
        else:                                              # libjpeg has no upsampler for the layout
            assert st == 2 and colour == VSF_ERR_INVALID_ARG, name
