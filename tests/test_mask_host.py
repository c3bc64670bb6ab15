"""Detection masks, host side, no GPU: the C ABI exports the calls, the binding lists them, the header states the slot limit the
binding uses, and the argument checks that need no context answer VSF_ERR_INVALID_ARG.

A context cannot exist without a device (vsf_create answers VSF_ERR_NO_DEVICE), so what a context's defaults ARE -- (-1, -1) for
vsf_get_image_masks, no slot set -- is asserted where one exists, in tests/test_gpu_mask.py; here only that the binding's "no
mask" is the header's -1."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

MASK_CALLS = ("vsf_mask_set", "vsf_mask_set_dev", "vsf_mask_clear", "vsf_mask_is_set", "vsf_mask_slot_bytes",
              "vsf_set_image_masks", "vsf_get_image_masks", "vsf_debug_mask_level", "vsf_observe_set_stream_masks")


@pytest.fixture(scope="module")
def capi():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as g
    from vision_slam_frontend_amd import capi
    if not capi.LIB_PATH.exists():
        g.build()
    return capi


def test_mask_calls_are_exported_and_listed(capi):
    lib = ctypes.CDLL(str(capi.LIB_PATH))
    for name in MASK_CALLS:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS, name


def test_slot_limit_serves_32_streams_of_two_eyes(capi):
    header = (ROOT / "include" / "vsf.h").read_text()
    limit = int(re.search(r"#define VSF_MAX_MASKS (\d+)", header).group(1))
    assert limit == capi.MAX_MASKS >= 32 * 2
    assert capi.NO_MASK == -1
    assert "restated from memory" in header.lower() and "orb.cpp / keypoint.cpp" in header


def test_argument_checks_without_a_context(capi):
    L = capi.lib()
    mask = np.full((8, 8), 255, np.uint8)
    p = mask.ctypes.data_as(ctypes.c_void_p)
    a, b = ctypes.c_int(7), ctypes.c_int(7)
    n = ctypes.c_size_t(7)
    inv = capi.VSF_ERR_INVALID_ARG
    assert L.vsf_mask_set(None, 0, p, 8, 8, 8) == inv
    assert L.vsf_mask_set_dev(None, 0, p, 8, 8, 8) == inv
    assert L.vsf_mask_clear(None, 0) == inv
    assert L.vsf_mask_is_set(None, 0, ctypes.byref(a)) == inv
    assert L.vsf_mask_slot_bytes(None, ctypes.byref(n)) == inv
    assert L.vsf_set_image_masks(None, -1, -1) == inv
    assert L.vsf_get_image_masks(None, ctypes.byref(a), ctypes.byref(b)) == inv
    assert L.vsf_debug_mask_level(None, 0, 0, p, 8) == inv
    assert L.vsf_observe_set_stream_masks(None, 0, -1, -1) == inv
    assert (a.value, b.value, n.value) == (7, 7, 7)  # nothing written
