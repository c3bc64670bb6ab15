"""The JPEG decoders on every sampling layout the host parser accepts (tests/jpeg_craft.py sampling_cases(): 4:4:0, 4:1:1,
4:1:0, luminance 3 x 1 .. 2 x 3, chroma components of several and of unequal block counts, and -- in files whose scans never
interleave -- luminance up to 4 x 4), in every process: one interleaved scan with and without restart intervals (the parallel
decoder; the one-wave decoder under vsf_debug_jpeg_serial), separate and partly interleaved sequential scans, and three
progressive scripts (the pipelined and the scan-after-scan kernel).  Bit for bit against the oracle and the system's libjpeg
(tests/test_jpeg_sampling_cases.py pins the two to each other and to Pillow on the CPU; tests/test_jpeg_sampling_plan.py shows
that each file reaches the decoder it is named for); reduced sizes against libjpeg at 1/2, 1/4, 1/8.  The destination has
poisoned padding behind every row and four poisoned guard rows below every image: blocks of the padded grid that lie wholly
outside the image must not be stored."""
import numpy as np
import pytest

import jpeg_craft as jc
import jpeg_ref
import jpeg_ref_reduced

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POISON = 0xEE
GUARD_ROWS = 4
ACCEPTED = jc.SAMPLING_INTERLEAVED + jc.SAMPLING_SEPARATE_ONLY


@pytest.fixture(scope="module")
def ctx():
    from vision_slam_frontend_amd import capi
    c = capi.Context(capi.default_params(640, 480, max_images=2, nfeatures=500))
    yield c
    c.close()


@pytest.fixture(scope="module")
def want(oracle):
    """{name: the oracle's pixels}, computed once and read-only; equal to the system's libjpeg where there is one."""
    out = {}
    for name, data, w, h, factors, process in jc.sampling_cases():
        img = oracle.jpeg_decode_gray(data)
        assert img.shape == (h, w), name
        if jpeg_ref.available():
            st, ref, warn = jpeg_ref.imdecode_gray(data, w, h)
            assert st == 0 and warn == 0, (name, st, warn)
            np.testing.assert_array_equal(img, ref, err_msg=name)
        img.setflags(write=False)
        out[name] = img
    return out


_reduced = {}


def want_reduced(name, data, d):
    """libjpeg's pixels at 1 / d (the rule of tests/test_gpu_jpeg_reduced.py: the library must be there), decoded once."""
    if (name, d) not in _reduced:
        assert jpeg_ref_reduced.available(), "no libjpeg.so.8 to build tests/cpp/jpeg_ref_reduced.c against"
        st, img, warn = jpeg_ref_reduced.imdecode_reduced_gray(data, d)
        assert st == 0 and warn == 0, (name, d, st, warn)
        img.setflags(write=False)
        _reduced[(name, d)] = img
    return _reduced[(name, d)]


def _decode(ctx, files, w, h, reduce=1, allow_status=()):
    """One call into a poisoned destination: pitch (w + 3) // 4 * 4 + 8, h + 4 rows per image.  -> (status, the whole buffer);
    after an accepted call the guard rows and the bytes behind each row must still be poison."""
    from vision_slam_frontend_amd import capi
    pitch, rows = (w + 3) // 4 * 4 + 8, h + GUARD_ROWS
    d = torch.full((len(files), rows, pitch), POISON, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    if reduce == 1:
        st = ctx.jpeg_decode_gray_batch(files, w, h, d.data_ptr(), rows * pitch, pitch, allow_status=allow_status)
    else:
        st = ctx.imdecode_reduced_gray_batch(files, reduce, w, h, d.data_ptr(), rows * pitch, pitch, allow_status=allow_status)
    assert ctx.sync() == capi.VSF_OK
    got = d.cpu().numpy()
    if st == capi.VSF_OK:
        assert (got[:, h:, :] == POISON).all(), "written below the image"
        # (full size: padding up to the row's last dword may be written; the reduced forms stop at the last pixel)
        assert (got[:, :h, ((w + 3) // 4 * 4 if reduce == 1 else w):] == POISON).all(), "written behind the row"
    return st, got


def _cases(factors=None, size=None, processes=None):
    return [c for c in jc.sampling_cases() if (factors is None or c[4] == factors) and (size is None or (c[2], c[3]) == size) and
            (processes is None or c[5] in processes)]


@pytest.mark.parametrize("factors", ACCEPTED, ids=jc.sampling_name)
def test_every_layout_every_process(ctx, want, factors):
    """One call per size with all of the set's processes, each file twice (the list, then the list again).  With the context as
    it is the one-scan files -- with restart intervals (their markers are in step) and without -- take the parallel decoder and
    the others jpeg_prog_pipe_kernel, in one upload.  Then again under vsf_debug_jpeg_serial: the host plans with force_serial
    (every one-scan file to the one-wave jpeg_gray_kernel) and the launcher gets prog_serial, which skips
    jpeg_prog_pipe_kernel, so the progressive and multi-scan files run through jpeg_prog_kernel alone (with the table
    expansion in front of it and jpeg_idct_kernel behind)."""
    from vision_slam_frontend_amd import capi
    try:
        for serial in (False, True):
            ctx.debug_jpeg_serial(serial)
            for size in ((75, 61), (96, 96), (25, 9), (1, 1)):
                cases = _cases(factors, size)
                assert cases
                files = [c[1] for c in cases] * 2
                st, got = _decode(ctx, files, *size)
                assert st == capi.VSF_OK
                for i in range(len(files)):
                    name = cases[i % len(cases)][0]
                    np.testing.assert_array_equal(got[i, :size[1], :size[0]], want[name],
                                                  err_msg="%s, position %d, serial %d" % (name, i, serial))
    finally:
        ctx.debug_jpeg_serial(False)


def _mixed_list():
    """75 x 61, every accepted set (the one-component ones included) in four processes, ordered so that neighbours differ in
    their luminance block count: smallest, largest, second smallest ..."""
    sets = sorted(ACCEPTED + jc.SAMPLING_GRAY, key=lambda f: (f[0][0] * f[0][1] if len(f) > 1 else 1, f))
    order = []
    while sets:
        order.append(sets.pop(0))
        if sets:
            order.append(sets.pop())
    out = []
    for round_ in range(4):
        for factors in order:
            have = {c[5]: c for c in _cases(factors, (75, 61))}
            if len(factors) == 1:
                pick = ["base", "base_rst", "prog_sep", None][round_]
            elif "base" in have:
                pick = ["base", "base_rst", "prog_il", "multi_sep"][round_]
            else:
                pick = [None, None, "prog_sep", "multi_sep"][round_]
            if pick:
                out.append(have[pick])
    return out


def test_mixed_layouts_in_one_batch(ctx, want):
    """The coefficient buffer's slots are sized by the largest file of the call (108 blocks: 4 x 3 luminance in 3 x 3 MCUs), every file's
    decoder and IDCT walk its own grid inside its slot.  The list, then the list reversed."""
    from vision_slam_frontend_amd import capi
    cases = _mixed_list()
    assert len(cases) == 13 * 4 + 5 * 2 + 2 * 3
    lums = [c[4][0][0] * c[4][0][1] if len(c[4]) > 1 else 1 for c in cases]
    assert sum(a != b for a, b in zip(lums, lums[1:])) >= len(lums) - 8
    for order in (cases, cases[::-1]):
        st, got = _decode(ctx, [c[1] for c in order], 75, 61)
        assert st == capi.VSF_OK
        for i, c in enumerate(order):
            np.testing.assert_array_equal(got[i, :61, :75], want[c[0]], err_msg="%s at position %d" % (c[0], i))


@pytest.mark.parametrize("d", [2, 4, 8])
def test_reduced_sizes(ctx, d):
    """store_reduced_packed (the one-wave decoder: groups of 15, 12 and 9 parked blocks, groups that begin in the middle of a
    dword) and jpeg_idct_reduced_kernel's block_at (units of D / 2 blocks that straddle MCUs of 3 blocks a row), at 75 x 61 and
    96 x 96, against libjpeg at 1 / d."""
    from vision_slam_frontend_amd import capi
    try:
        for serial in (False, True):
            ctx.debug_jpeg_serial(serial)
            for factors in ACCEPTED:
                for size in ((75, 61), (96, 96)):
                    cases = _cases(factors, size, ("base", "base_rst", "prog_sep", "prog_il"))
                    assert cases
                    w, h = jpeg_ref_reduced.reduced_size(size[0], size[1], d)
                    st, got = _decode(ctx, [c[1] for c in cases], w, h, reduce=d)
                    assert st == capi.VSF_OK
                    for i, c in enumerate(cases):
                        np.testing.assert_array_equal(got[i, :h, :w], want_reduced(c[0], c[1], d),
                                                      err_msg="%s at 1/%d, serial %d" % (c[0], d, serial))
    finally:
        ctx.debug_jpeg_serial(False)


def test_parallel_decoder_long_segments(ctx, want):
    """640 x 480 one-scan files of 5, 10 and 10 blocks per MCU beside a 4:2:0 control: each of the parallel decoder's 256
    segments holds at least 16 blocks, so the merge marks at 2, 4, 8 and 16 blocks are set and met with the block-in-MCU
    state wrapping at 5 and 10."""
    from vision_slam_frontend_amd import capi
    cases = _cases(size=(640, 480))
    assert [c[4] for c in cases] == jc.SAMPLING_LONG + [jc.SAMPLING_CONTROL]
    for c in cases:
        m = sum(fh * fv for fh, fv in c[4])
        assert -(-640 // (8 * c[4][0][0])) * -(-480 // (8 * c[4][0][1])) * m >= 16 * 256
    st, got = _decode(ctx, [c[1] for c in cases], 640, 480)
    assert st == capi.VSF_OK
    for i, c in enumerate(cases):
        np.testing.assert_array_equal(got[i, :480, :640], want[c[0]], err_msg=c[0])


def test_refusals(ctx, want):
    """More than 10 blocks in an interleaved MCU: VSF_ERR_INVALID_ARG (libjpeg refuses too); a luminance component below the
    largest factors: VSF_ERR_UNSUPPORTED (libjpeg upsamples it).  Alone and behind a good file; nothing is written, and the
    next good call is exact."""
    from vision_slam_frontend_amd import capi
    good = _cases(jc.SAMPLING_INTERLEAVED[0], (75, 61), ("base",))[0]
    refusals = jc.sampling_refusals()
    assert len({r[4] for r in refusals}) == 5
    for name, data, w, h, factors, process, answer in refusals:
        expect = capi.VSF_ERR_INVALID_ARG if answer == "invalid_arg" else capi.VSF_ERR_UNSUPPORTED
        for files in ([data], [good[1], data]):
            st, got = _decode(ctx, files, w, h, allow_status=range(1, 6))
            assert st == expect, (name, st)
            assert (got == POISON).all(), name
    st, got = _decode(ctx, [good[1]], 75, 61)
    assert st == capi.VSF_OK
    np.testing.assert_array_equal(got[0, :61, :75], want[good[0]])


def test_gray_files_with_factors(ctx, want):
    """One-component files whose SOF names 2 x 2 and 3 x 1: one block per MCU whatever the factors say (T.81 A.2.2).  All
    three processes, full size and reduced, both decoders."""
    from vision_slam_frontend_amd import capi
    try:
        for serial in (False, True):
            ctx.debug_jpeg_serial(serial)
            for factors in jc.SAMPLING_GRAY:
                for size in ((75, 61), (96, 96), (25, 9), (1, 1)):
                    cases = _cases(factors, size)
                    assert len(cases) == (3 if size == (75, 61) else 2)
                    files = [c[1] for c in cases] * 2
                    st, got = _decode(ctx, files, *size)
                    assert st == capi.VSF_OK
                    for i in range(len(files)):
                        c = cases[i % len(cases)]
                        np.testing.assert_array_equal(got[i, :size[1], :size[0]], want[c[0]], err_msg="%s, serial %d" % (c[0], serial))
                    for d in (2, 4, 8):
                        w, h = jpeg_ref_reduced.reduced_size(size[0], size[1], d)
                        st, got = _decode(ctx, [c[1] for c in cases], w, h, reduce=d)
                        assert st == capi.VSF_OK
                        for i, c in enumerate(cases):
                            np.testing.assert_array_equal(got[i, :h, :w], want_reduced(c[0], c[1], d),
                                                          err_msg="%s at 1/%d, serial %d" % (c[0], d, serial))
    finally:
        ctx.debug_jpeg_serial(False)
