"""cv::resize on the device, the parts that need none: csrc/vsf_resize.h's taps against the oracle's tables
(oracle.binding.resize_tables) for the size pairs tests/test_gpu_resize.py runs, and the arithmetic of the ObserveImage queue's
declared input sizes (csrc/vsf_observe_plan.cc: the big slots, the runs a resize launch takes, the raw frames' upload span) --
from Python through a small library (tests/cpp/resize_plan_capi.cc), and as a stand-alone program
(tests/cpp/test_observe_resize_plan.cc) built plainly and under AddressSanitizer + UBSan.  Nothing sanitised is loaded here."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
PLAN_CC = str(ROOT / "vision_slam_frontend_amd" / "csrc" / "vsf_observe_plan.cc")
PAIRS = [((128, 96), (64, 48)), ((129, 97), (64, 48)), ((192, 144), (64, 48)), ((512, 384), (64, 48)), ((100, 80), (64, 48)),
         ((40, 30), (64, 48)), ((64, 48), (64, 48)), ((131, 67), (61, 47)), ((7, 5), (3, 2)), ((7, 5), (1, 1)),
         ((1300, 40), (520, 16)), ((2600, 24), (520, 10)), ((10400, 9), (260, 4)), ((130, 9), (523, 20)),
         ((1280, 960), (640, 480)), ((1920, 1080), (640, 360)), ((641, 481), (320, 240))]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("resize_plan") / "libresize_plan.so"
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so),
                        str(ROOT / "tests" / "cpp" / "resize_plan_capi.cc"), PLAN_CC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    L = C.CDLL(str(so))
    vp, i32, u64 = C.c_void_p, C.c_int32, C.c_uint64
    L.t_resize_taps.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.t_resize_taps.restype = None
    L.t_resize_span_dwords.argtypes = [i32, i32]
    for f, a in ((L.t_input_pitch, [i32]), (L.t_input_image_bytes, [i32, i32]), (L.t_input_half_bytes, [vp, vp, i32]),
                 (L.t_input_ring_bytes, [i32, u64])):
        f.argtypes, f.restype = a, u64
    L.t_resize_plan.argtypes = [vp, i32, C.c_int64, i32, i32, vp, i32, vp, vp]
    L.t_upload_max_gap.argtypes = [u64]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("pair", PAIRS, ids=["%dx%d-%dx%d" % (s + d) for s, d in PAIRS])
def test_taps_equal_the_oracles_tables(lib, pair):
    """xofs / ialpha as they are; yofs clipped into the image as resizeGeneric_Invoker clips the row pointers, ibeta kept; where
    the oracle takes its single-tap branch (dx >= xmax) the taps carry weight 2048 on S[xofs] and 0 on a pixel inside the row."""
    from oracle import binding as ob
    (sw, sh), (dw, dh) = pair
    xofs, ia, yofs, ib, xmax = ob.resize_tables(sw, sh, dw, dh)
    x0, x1, yo0, yo1 = (np.empty(n, np.int32) for n in (dw, dw, dh, dh))
    a, b = np.empty(2 * dw, np.int16), np.empty(2 * dh, np.int16)
    lib.t_resize_taps(sw, sh, dw, dh, _p(x0), _p(x1), _p(a), _p(yo0), _p(yo1), _p(b))
    assert np.array_equal(x0, xofs) and np.array_equal(a, ia) and np.array_equal(b, ib)
    assert np.array_equal(yo0, np.clip(yofs, 0, sh - 1)) and np.array_equal(yo1, np.clip(yofs + 1, 0, sh - 1))
    assert (x1 < sw).all() and (x1[:xmax] == xofs[:xmax] + 1).all()
    assert (a[0::2][xmax:] == 2048).all() and (a[1::2][xmax:] == 0).all()
    need = lib.t_resize_span_dwords(sw, dw)
    for xb in range(0, dw, 256):  # every tap of a wave's 256 columns inside the window the launch sizes, at any skew
        xe = min(xb + 255, dw - 1)
        assert x0[xb:xe + 1].min() >= x0[xb] and (x1[xb:xe + 1].max() - x0[xb]) + 3 < 4 * need


def test_slots_and_rings(lib):
    assert lib.t_input_pitch(640) == 640 and lib.t_input_pitch(641) == 704 and lib.t_input_pitch(0) == 0
    assert lib.t_input_image_bytes(1280, 960) == 1280 * 960 and lib.t_input_image_bytes(200, 150) == 256 * 150
    w, h = np.array([1280, 0, 640], np.int32), np.array([960, 0, 480], np.int32)
    half = lib.t_input_half_bytes(_p(w), _p(h), 3)
    assert half == 1280 * 960 and lib.t_input_half_bytes(_p(w[1:]), _p(h[1:]), 1) == 0
    # what include/vsf.h quotes: depth 256 at 1280 x 960
    assert lib.t_input_ring_bytes(256, half) == 256 * 2 * 1280 * 960 == 629145600


def test_resize_runs(lib):
    def plan(frames, t0, depth, max_gap=3):
        """-> (runs, uploads as [f0, n, slot0], frames resized)"""
        a = np.array(frames, np.int32).reshape(-1, 3)
        runs, ups, counts = np.zeros((len(a), 6), np.int32), np.zeros((len(a), 3), np.int32), np.zeros(2, np.int32)
        n = lib.t_resize_plan(_p(a), len(a), t0, depth, max_gap, _p(runs), len(a), _p(ups), _p(counts))
        return (None, None, None) if n < 0 else (runs[:n].tolist(), ups[:counts[0]].tolist(), int(counts[1]))

    big, small, none, DEV, PNG = (640, 480), (200, 150), (0, 0), 3, 2
    # an interleaved group of cameras: big raw, small png, none, big device -- twice; depth 8 from ticket 6 (wraps after 2)
    frames = [big + (0,), small + (PNG,), none + (0,), big + (DEV,)] * 2
    runs, ups, resized = plan(frames, 6, 8)
    assert runs == [[0, 0, 1, 0, 640, 480], [0, 1, 1, 1, 200, 150], [1, 3, 1, 1, 640, 480], [0, 4, 1, 4, 640, 480],
                    [0, 5, 1, 5, 200, 150], [1, 7, 1, 5, 640, 480]]
    # raw frames 0 (slot 6) and 4 (slot 2): the gap of three slots is worth bridging, but the ring wraps inside it
    assert ups == [[0, 1, 6], [4, 1, 2]] and resized == 6
    # ... from ticket 0 it does not: ONE upload of five slots at a gap of three allowed, two uploads at two
    assert plan(frames, 0, 8)[1] == [[0, 5, 0]] and plan(frames, 0, 8, max_gap=2)[1] == [[0, 1, 0], [4, 1, 4]]
    # what a gap may be: what the link carries in a copy command's fixed cost, over the slot (1280 x 960: 3 slots)
    assert lib.t_upload_max_gap(2 * 1280 * 960) == 3 and lib.t_upload_max_gap(2 * 640 * 480) == 14
    # one camera: one run, however the frames came in; device frames are cut where their ring wraps
    assert plan([big + (0,)] * 5, 0, 8)[0] == [[0, 0, 5, 0, 640, 480]]
    assert plan([big + (DEV,)] * 5, 6, 8)[0] == [[1, 0, 2, 6, 640, 480], [1, 2, 3, 0, 640, 480]]
    assert plan([none + (0,)] * 3, 0, 8) == ([], [], 0)
    assert plan([(640, 0, 0)], 0, 8)[0] is None and plan([big + (0,)] * 3, 0, 2)[0] is None


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_resize_plan_program(tmp_path, flags):
    exe = tmp_path / "test_observe_resize_plan"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", str(exe),
                        str(ROOT / "tests" / "cpp" / "test_observe_resize_plan.cc"), PLAN_CC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])
