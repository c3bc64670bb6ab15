"""vsf_params::score_type without a GPU: which values vsf_create takes, and the keypoint room of both modes
(vsf_debug_level_room: the geometry vsf_create itself would build, host only)."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from vision_slam_frontend_amd import capi
    if not capi.LIB_PATH.exists():
        g.build()
    return capi


def _create(capi, p):
    h = ctypes.c_void_p()
    st = capi.lib().vsf_create(ctypes.byref(p), 0, ctypes.byref(h))
    if st == capi.VSF_OK:
        capi.lib().vsf_destroy(h)
    return st


def test_create_takes_harris_and_fast_score_only(capi):
    import torch
    have_gpu = torch.cuda.is_available()
    assert (capi.HARRIS_SCORE, capi.FAST_SCORE) == (0, 1)
    assert capi.default_params(640, 480).score_type == capi.HARRIS_SCORE  # vsf_params_default: the reference's literal
    for score_type in (0, 1):
        st = _create(capi, capi.default_params(640, 480, nfeatures=2000, score_type=score_type))
        # past the parameter check: a context where there is a device, "no usable GPU" where there is none
        assert st == (capi.VSF_OK if have_gpu else capi.VSF_ERR_NO_DEVICE), (score_type, st)
    for score_type in (2, -1, 3, 1 << 20):
        assert _create(capi, capi.default_params(640, 480, score_type=score_type)) == capi.VSF_ERR_UNSUPPORTED
    # the other three single-valued arguments stay as they were, in either mode
    for over in (dict(wta_k=3), dict(wta_k=4), dict(patch_size=15), dict(first_level=1)):
        for score_type in (0, 1):
            assert _create(capi, capi.default_params(640, 480, score_type=score_type, **over)) == capi.VSF_ERR_UNSUPPORTED


def _budget(nfeatures, scale_factor, nlevels):
    """computeKeyPoints' per-level budget, restated (float arithmetic as OpenCV's)."""
    f32 = np.float32
    factor = f32(1.0 / float(f32(scale_factor)))
    nd = f32(nfeatures) * (f32(1) - factor) / (f32(1) - f32(float(factor) ** nlevels))
    out, total = [], 0
    for _ in range(nlevels - 1):
        out.append(int(np.rint(nd)))
        total += out[-1]
        nd = f32(nd * factor)
    out.append(max(nfeatures - total, 0))
    return out


CASES = [(640, 480, 2000, 1.04, 50), (640, 480, 10000, 1.04, 50), (640, 480, 500, 1.2, 8), (160, 120, 300, 1.2, 8)]


@pytest.mark.parametrize("w,h,nf,sf,nl", CASES)
def test_harris_geometry_is_unchanged(capi, w, h, nf, sf, nl):
    """A level holds 2 n_l + 64 records whatever max_keypoints says: 7 200 records per image at (2000, 1.04, 50)."""
    budget = _budget(nf, sf, nl)
    for mk in (0, nf + 1024, 777):
        room, nfeat, total = capi.level_room(capi.default_params(w, h, nfeatures=nf, scale_factor=sf, nlevels=nl, max_keypoints=mk))
        assert nfeat.tolist() == budget and sum(budget) == nf
        assert room.tolist() == [2 * n + 64 for n in budget]
        assert total == 2 * nf + 64 * nl
    if (nf, nl) == (2000, 50):
        assert total == 7200


@pytest.mark.parametrize("w,h,nf,sf,nl", CASES)
def test_fast_score_room_rule(capi, w, h, nf, sf, nl):
    """include/vsf.h: a level holds n_l + max(max_keypoints - nfeatures, 0), max_keypoints = 0 standing for nfeatures + 256."""
    budget = _budget(nf, sf, nl)
    for mk, headroom in ((0, 256), (nf + 256, 256), (nf + 1024, 1024), (nf, 0), (nf - 100, 0), (nf + 1, 1)):
        p = capi.default_params(w, h, nfeatures=nf, scale_factor=sf, nlevels=nl, max_keypoints=mk, score_type=capi.FAST_SCORE)
        room, nfeat, total = capi.level_room(p)
        assert nfeat.tolist() == budget
        assert room.tolist() == [n + headroom for n in budget], (mk, headroom)
        assert total == nf + headroom * nl
    if (nf, nl) == (2000, 50):  # default headroom: 14 800 records per image against HARRIS mode's 7 200
        assert capi.level_room(capi.default_params(w, h, nfeatures=nf, score_type=1))[2] == 14800


def test_named_cases_against_the_rule(capi):
    """The capacity cases of tests/test_gpu_score_type.py as arithmetic (figures: tests/test_orb_score_ref.py)."""
    room, nfeat, _ = capi.level_room(capi.default_params(640, 480, nfeatures=2000, score_type=1))
    assert (nfeat[2], room[2]) == (83, 339) and 83 + 439 > room[2] and 2388 > 2000 + 256  # checkerboard(8), default: overflows
    room, _, _ = capi.level_room(capi.default_params(640, 480, nfeatures=2000, max_keypoints=3024, score_type=1))
    assert room[2] == 83 + 1024 >= 83 + 439 and 2698 <= 3024                                # ... nfeatures + 1024 holds it
    room, nfeat, _ = capi.level_room(capi.default_params(640, 480, nfeatures=500, scale_factor=1.2, nlevels=8, score_type=1))
    assert (nfeat[0], room[0]) == (109, 365) and 173 <= room[0] and 617 <= 756              # line_art at (1.2, 8, 500): fits


def test_level_room_checks_its_arguments(capi):
    L = capi.lib()
    total = ctypes.c_int64()
    p = capi.default_params(640, 480, score_type=2)
    room = np.zeros(64, np.int32)
    assert L.vsf_debug_level_room(ctypes.byref(p), room.ctypes.data, None, 64, ctypes.byref(total)) == capi.VSF_ERR_UNSUPPORTED
    p = capi.default_params(640, 480)
    assert L.vsf_debug_level_room(None, room.ctypes.data, None, 64, ctypes.byref(total)) == capi.VSF_ERR_INVALID_ARG
    assert L.vsf_debug_level_room(ctypes.byref(p), None, None, 64, ctypes.byref(total)) == capi.VSF_ERR_INVALID_ARG
    assert L.vsf_debug_level_room(ctypes.byref(p), room.ctypes.data, None, 64, None) == capi.VSF_ERR_INVALID_ARG
    assert L.vsf_debug_level_room(ctypes.byref(p), room.ctypes.data, None, 3, ctypes.byref(total)) == capi.VSF_OK
    assert room[3] == 0 and room[2] > 0 and total.value == 2 * 10000 + 64 * 50
