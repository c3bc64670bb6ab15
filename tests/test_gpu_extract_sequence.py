"""Every scheduling mechanism of the extraction (csrc/vsf_extract_plan.h, csrc/vsf_api.hip extract_on) in ONE context's life,
one after the other -- the other GPU tests exercise each alone.  One context makes this sequence of vsf_stereo_batch_dev calls,
each on an image set of its own:

1. two pipelined calls with VSF_OPT_FAST_EARLY_LEVELS 2 and VSF_OPT_BLUR_EARLY 1;
2. a 16-image call (the blur in line, buffer 0);
3. a two-lane call (vsf_set_lanes 2 and back);
4. vsf_tune_fast_resident (the forced FAST forms, no early part; later 32-image calls take what it measured);
5. a call with early levels 0 and blur-early 0;
6. pipelining off for one call and on again;
7. two more calls with early levels 2 and blur-early 1.

Keypoints, descriptors, counts, matches and match counts of EVERY call must be byte for byte what a fresh context that never
pipelines returns for the same images (the tune call returns no matches: its keypoints, descriptors and counts are compared),
and after the last call debug_level_image must give one plain and one blurred level as the CPU oracle has them: the hooks
follow the buffers the last call wrote.

Shape: 352x160, 32 images (16 stereo frames), 500 features -- by tests/test_gpu_fast_split.py the smallest image with a
full-width FAST cell and the smallest batch whose blur runs beside FAST.  In the 8-level / 1.2 pyramid only level 0 has such a
cell (the early part is clamped to it and starts before the chain's first launch); in the 50-level / 1.04 pyramid levels 0..2
have, and the early part starts behind the launch that makes level 1."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, B, NF = 352, 160, 16, 500
SMALL = 8  # frames of the 16-image call
NAMES = ("kp", "desc", "counts", "matches", "nmatches")
PYRAMIDS = [(8, 1.2), (50, 1.04)]
# (what the call is, frames); one image set per entry
STEPS = [("early", B), ("early", B), ("plain", SMALL), ("lanes", B), ("tune", B), ("late", B), ("unpipelined", B), ("early", B),
         ("early", B)]


@pytest.fixture(scope="module")
def capi():
    from vision_slam_frontend_amd import capi
    capi.lib()
    return capi


@pytest.fixture(scope="module")
def sets():
    from vision_slam_frontend_amd import synth
    return [synth.bench_batch(B, W, H, seed=synth.BASE_SEED + 230 + k, n_scenes=4)[:frames] for k, (_, frames) in enumerate(STEPS)]


def _levels_with_a_full_cell(capi, params):
    words = np.zeros(1 << 18, np.uint32)
    levels = np.zeros((64, 10), np.int32)
    nw, nf = C.c_int(), C.c_int()
    assert capi.lib().vsf_debug_fast_work(C.byref(params), 1, 1, words.ctypes.data, 1 << 18, C.byref(nw), C.byref(nf),
                                          levels.ctypes.data, 64) == capi.VSF_OK
    full = set()
    for wd in words[:nf.value]:
        l, b = int(wd >> 24), int((wd >> 16) & 0xFF)
        x_hi, a0 = int(levels[l][3]), int(levels[l][6])
        if (min(x_hi, a0 + 248 * (b + 1)) - (a0 + 248 * b) + 3) // 4 + 2 >= 64:
            full.add(l)
    return full


def _run(capi, sets, pyramid, mixed, levels_of=()):
    """mixed: the sequence of the docstring; not mixed: every image set through a plain call of a context that never pipelines.
    -> per step the output arrays, and {(level, blurred): image} of image 2 B - 1 of the last call for levels_of."""
    import torch
    dev = torch.device("cuda", 0)
    nlevels, scale = pyramid
    params = capi.default_params(W, H, max_images=2 * B, nfeatures=NF, nlevels=nlevels, scale_factor=scale)
    if mixed:
        assert 0 in _levels_with_a_full_cell(capi, params), "no full FAST cell: no call would have an early part"
    with capi.Context(params) as ctx:
        K = ctx.params.max_keypoints
        d_img = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in sets]
        outs = [(torch.zeros((2 * n, K, 28), dtype=torch.uint8, device=dev), torch.zeros((2 * n, K, 32), dtype=torch.uint8, device=dev),
                 torch.zeros(2 * n, dtype=torch.int32, device=dev), torch.zeros((n, K, 16), dtype=torch.uint8, device=dev),
                 torch.zeros(n, dtype=torch.int32, device=dev)) for _, n in STEPS]
        torch.cuda.synchronize()

        def early(levels, blur):
            ctx.set_option(capi.OPT_FAST_EARLY_LEVELS, levels)
            ctx.set_option(capi.OPT_BLUR_EARLY, blur)

        def call(c):
            ctx.stereo_batch_dev(d_img[c].data_ptr(), STEPS[c][1], W * H, W, *[t.data_ptr() for t in outs[c]])

        if mixed:
            ctx.set_pipeline(True)
        for c, (what, n) in enumerate(STEPS):
            if not mixed:
                call(c)
            elif what == "early":
                early(2, 1)
                call(c)
            elif what == "plain":
                call(c)
            elif what == "lanes":
                ctx.set_lanes(2)
                call(c)
                ctx.set_lanes(1)
            elif what == "tune":
                ctx.tune_fast_resident(d_img[c].data_ptr(), 2 * n, W * H, W, *[t.data_ptr() for t in outs[c][:3]], samples=1)
            elif what == "late":
                early(0, 0)
                call(c)
            elif what == "unpipelined":
                ctx.set_pipeline(False)
                call(c)
                ctx.set_pipeline(True)
        assert ctx.sync() == capi.VSF_OK
        torch.cuda.synchronize()
        images = {(l, blurred): ctx.debug_level_image(2 * B - 1, l, blurred) for l, blurred in levels_of}
        res = [[t.cpu().numpy() for t in o] for o in outs]
    return res, images


@pytest.mark.parametrize("pyramid", PYRAMIDS, ids=["8x1.2", "50x1.04"])
def test_mixed_sequence(capi, oracle, sets, pyramid):
    nlevels, scale = pyramid
    levels_of = ((3, False), (2, True))
    ref, _ = _run(capi, sets, pyramid, False)
    got, images = _run(capi, sets, pyramid, True, levels_of)
    assert int(ref[0][2].min()) > 50, "the scene gives too few keypoints to tell anything"
    for c, (what, _) in enumerate(STEPS):
        for name, a, b in list(zip(NAMES, ref[c], got[c]))[:3 if what == "tune" else 5]:
            assert a.tobytes() == b.tobytes(), "call %d (%s): %s differs" % (c, what, name)
    o = oracle.Orb(nfeatures=NF, nlevels=nlevels, scale_factor=scale)
    o.run(sets[-1][B - 1, 1])
    for l, blurred in levels_of:
        np.testing.assert_array_equal(images[(l, blurred)], o.level_image(l, blurred), err_msg="level %d blurred %r" % (l, blurred))
