"""The references of tests/test_gpu_jpeg_sampling.py, pinned on the CPU: every file of jpeg_craft.sampling_cases() -- sampling
factors beyond 4:4:4 / 4:2:2 / 4:2:0, in one interleaved scan, in separate scans and progressive -- is read by the system's
libjpeg (tests/jpeg_ref.py) without a warning, to the pixels the oracle gives and, where Pillow is there, to the pixels its
libjpeg-turbo gives; libjpeg also reads each at 1/2, 1/4 and 1/8 without a warning (tests/jpeg_ref_reduced.py).  The refusal
files: libjpeg refuses the ones whose interleaved MCU exceeds 10 blocks and decodes the ones whose luminance it upsamples."""
import io

import numpy as np
import pytest

import jpeg_craft as jc
import jpeg_ref
import jpeg_ref_reduced


def _need_libjpeg():
    if not jpeg_ref.available():
        pytest.skip("no libjpeg.so.8 to build tests/cpp/jpeg_ref.c against")


def test_the_case_table():
    """What the generator promises: every set in every process it can have, names unique, block counts as stated."""
    cases = jc.sampling_cases()
    assert len({c[0] for c in cases}) == len(cases)
    by_set = {}
    for name, data, w, h, factors, process in cases:
        by_set.setdefault(factors, set()).add((w, h, process))
    assert set(by_set) == set(jc.SAMPLING_INTERLEAVED + jc.SAMPLING_SEPARATE_ONLY + jc.SAMPLING_GRAY + [jc.SAMPLING_CONTROL])
    for factors in jc.SAMPLING_INTERLEAVED:
        assert sum(fh * fv for fh, fv in factors) <= 10
        have = by_set[factors]
        for p in ("base", "base_rst", "multi_sep", "prog_il", "prog_sep", "prog_mix"):
            assert (75, 61, p) in have, (factors, p)
        assert {(96, 96, "base"), (96, 96, "prog_il"), (25, 9, "base"), (25, 9, "prog_sep"), (1, 1, "base"), (1, 1, "prog_sep")} <= have
        assert ((75, 61, "multi_y_cb") in have) == (factors[0][0] * factors[0][1] + factors[1][0] * factors[1][1] <= 10)
    for factors in jc.SAMPLING_SEPARATE_ONLY:
        assert sum(fh * fv for fh, fv in factors) > 10 and factors[0][0] * factors[0][1] <= 16
        assert {p for w, h, p in by_set[factors]} == {"multi_sep", "prog_sep"}
    assert sum(fh * fv for fh, fv in jc.SAMPLING_INTERLEAVED[5]) == 10 and jc.SAMPLING_INTERLEAVED[5][0] == (4, 2)
    assert sum(fh * fv for fh, fv in jc.SAMPLING_INTERLEAVED[11]) == 10
    for factors in jc.SAMPLING_LONG:
        assert (640, 480, "base") in by_set[factors]
    assert sum(1 for c in cases if c[2] == 640) == 4
    # restart interval 3 at 75 x 61: intervals cross MCU rows wherever h < 4 (10, 5 and 4 MCUs a row; h = 4 has rows of 3)
    assert [-(-75 // (8 * fh)) for fh in (1, 2, 3, 4)] == [10, 5, 4, 3]
    ref = jc.sampling_refusals()
    assert len(ref) == 10 and {r[6] for r in ref} == {"invalid_arg", "unsupported"}


@pytest.mark.parametrize("factors", jc.SAMPLING_INTERLEAVED + jc.SAMPLING_SEPARATE_ONLY + jc.SAMPLING_GRAY + [jc.SAMPLING_CONTROL],
                         ids=jc.sampling_name)
def test_libjpeg_the_oracle_and_pillow_agree(oracle, factors):
    _need_libjpeg()
    try:
        from PIL import Image
    except ImportError:
        Image = None
    cases = [c for c in jc.sampling_cases() if c[4] == factors]
    assert cases
    for name, data, w, h, _, process in cases:
        st, ref, warn = jpeg_ref.imdecode_gray(data, w, h)
        assert st == 0 and warn == 0, (name, st, warn)
        assert ref.shape == (h, w)
        np.testing.assert_array_equal(oracle.jpeg_decode_gray(data), ref, err_msg=name)
        if Image is not None:
            im = Image.open(io.BytesIO(data))
            im.draft("L", im.size)
            np.testing.assert_array_equal(np.asarray(im.convert("L") if im.mode != "L" else im), ref, err_msg=name)
        if w * h > 1:
            assert ref.std() > 3, name   # (a picture, not a flat field)
        for d in (2, 4, 8):
            st, img, warn = jpeg_ref_reduced.imdecode_reduced_gray(data, d)
            assert st == 0 and warn == 0, (name, d, st, warn)
            assert img.shape == (-(-h // d), -(-w // d)), (name, d)


def test_what_libjpeg_does_with_the_refusals():
    _need_libjpeg()
    for name, data, w, h, factors, process, answer in jc.sampling_refusals():
        st, ref, warn = jpeg_ref.imdecode_gray(data, w, h)
        if answer == "invalid_arg":   # JERR_BAD_MCU_SIZE: more than 10 blocks in an interleaved MCU
            assert sum(fh * fv for fh, fv in factors) > 10
            assert st in (1, 2) and ref is None, (name, st)
        else:                         # libjpeg upsamples the luminance: a deviation include/vsf.h names
            assert st == 0 and warn == 0 and ref.shape == (h, w), (name, st, warn)
