"""VSF_OPT_FAST_EARLY_LEVELS on the GPU: a pipelined call scores the full cells of its first pyramid levels in a launch
of its own, queued from inside the call's pyramid chain onto the blur stream, into the other of two pairs of candidate
buffers, beside the previous call's selection.  Nothing a call returns may depend on it:

* five consecutive pipelined vsf_stereo_batch_dev calls on three batches in rotation, early levels 1, 2 and every level
  that has a full cell, FAST as a grid and resident (late part) with the early part as a grid and resident with 1..3 waves
  per SIMD -- keypoints, descriptors, counts and matches of EVERY call byte for byte what the same sequence gives with the
  option 0, and the FAST candidates of the last call for every level of two images;
* the option changed between calls (0 -> 2 -> 0 -> 3 -> 1): the buffer flip and the release events;
* 160x120, where no level has a full cell: the option is a no-op;
* one call of the first sequence against the CPU oracle (keypoints and descriptors, as tests/test_gpu_parity.py).

Shape: 352x160 -- the smallest kind of image whose levels 0..2 have a full-width cell (keypoint rectangle >= 245 columns)
and two strips each; confirmed below from the work list the library builds.  32 images, so that the blur runs beside FAST
and the resident form is eligible; 500 features."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, B, NF = 352, 160, 16, 500
CALLS = 5
NAMES = ("kp", "desc", "counts", "matches", "nmatches")


@pytest.fixture(scope="module")
def capi():
    from vision_slam_frontend_amd import capi
    capi.lib()
    return capi


def _full_levels(capi, w, h):
    """levels that have a full-width cell -> (their number, strips of each), from the library's own work list"""
    p = capi.default_params(w, h)
    words = np.zeros(1 << 18, np.uint32)
    levels = np.zeros((64, 10), np.int32)
    nw, nf = C.c_int(), C.c_int()
    assert capi.lib().vsf_debug_fast_work(C.byref(p), 1, 1, words.ctypes.data, 1 << 18, C.byref(nw), C.byref(nf),
                                          levels.ctypes.data, 64) == capi.VSF_OK
    full = set()
    for wd in words[:nf.value]:
        l, b = int(wd >> 24), int((wd >> 16) & 0xFF)
        x_hi, a0 = int(levels[l][3]), int(levels[l][6])
        if (min(x_hi, a0 + 248 * (b + 1)) - (a0 + 248 * b) + 3) // 4 + 2 >= 64:
            full.add(l)
    return full, levels


@pytest.fixture(scope="module")
def split_levels(capi):
    full, levels = _full_levels(capi, W, H)
    if not (len(full) >= 3 and full == set(range(len(full))) and all(int(levels[l][8]) >= 2 for l in full)):
        pytest.skip("%dx%d does not give three levels with a full-width FAST cell and two strips: %r" % (W, H, sorted(full)))
    return len(full)


def _batches(w, h):
    from vision_slam_frontend_amd import synth
    return [synth.bench_batch(B, w, h, seed=synth.BASE_SEED + 70 + k, n_scenes=4) for k in range(3)]


@pytest.fixture(scope="module")
def batches():
    return _batches(W, H)


def _sequence(capi, frames3, w, h, early, resident=0, early_form=0, candidates=True):
    """CALLS pipelined calls on the batches in rotation; `early`: the option's value for every call, or one value per call.
    -> per call the five output arrays, and the candidates of the last call: {(image, level): array}."""
    import torch
    dev = torch.device("cuda", 0)
    try:
        ctx = capi.Context(capi.default_params(w, h, max_images=2 * B, nfeatures=NF))
    except capi.VsfError as e:
        pytest.skip("the context rejects %dx%d: %s" % (w, h, e))
    with ctx:
        K = ctx.params.max_keypoints
        d_img = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames3]
        outs = [(torch.zeros((2 * B, K, 28), dtype=torch.uint8, device=dev), torch.zeros((2 * B, K, 32), dtype=torch.uint8, device=dev),
                 torch.zeros(2 * B, dtype=torch.int32, device=dev), torch.zeros((B, K, 16), dtype=torch.uint8, device=dev),
                 torch.zeros(B, dtype=torch.int32, device=dev)) for _ in range(CALLS)]
        torch.cuda.synchronize()
        ctx.set_pipeline(True)
        ctx.set_fast_resident(resident)
        ctx.set_option(capi.OPT_FAST_EARLY_FORM, early_form)
        per_call = list(early) if isinstance(early, (list, tuple)) else None
        if per_call is None:
            ctx.set_option(capi.OPT_FAST_EARLY_LEVELS, early)
            assert ctx.get_option(capi.OPT_FAST_EARLY_LEVELS) == early
        for c in range(CALLS):
            if per_call is not None:
                ctx.set_option(capi.OPT_FAST_EARLY_LEVELS, per_call[c])
            ctx.stereo_batch_dev(d_img[c % 3].data_ptr(), B, w * h, w, *[t.data_ptr() for t in outs[c]])
        assert ctx.sync() == capi.VSF_OK
        cands = {}
        if candidates:
            for image in (0, 2 * B - 1):
                for l in range(ctx.nlevels):
                    cands[(image, l)] = ctx.debug_fast_candidates(image, l, cap=w * h)
        res = [[t.cpu().numpy() for t in o] for o in outs]
    return res, cands


_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


@pytest.fixture(scope="module")
def reference(capi, batches, split_levels):
    return _sequence(capi, batches, W, H, 0)


def _same(ref, got, what):
    (r_out, r_cand), (g_out, g_cand) = ref, got
    for c in range(CALLS):
        for name, a, b in zip(NAMES, r_out[c], g_out[c]):
            assert a.tobytes() == b.tobytes(), "%s: call %d: %s differs" % (what, c, name)
    assert r_cand.keys() == g_cand.keys()
    for k in r_cand:
        assert r_cand[k].tobytes() == g_cand[k].tobytes(), "%s: candidates of image %d level %d" % ((what,) + k)


# (early levels: -1 = every level that has a full cell; FAST form of the late part; form of the early part)
CASES = [(1, 0, 0), (2, 0, 0), (-1, 0, 0), (1, 3, 2), (2, 3, 1), (-1, 3, 3), (2, 0, 3)]


@pytest.mark.parametrize("early,resident,early_form", CASES)
def test_byte_identity_across_the_split(capi, batches, split_levels, reference, early, resident, early_form):
    le = split_levels if early < 0 else early
    got = _cached((le, resident, early_form), lambda: _sequence(capi, batches, W, H, le, resident, early_form))
    assert int(got[0][0][2].min()) > 50 and sum(len(v) for v in got[1].values()) > 1000  # the scene gives FAST work
    _same(reference, got, "early levels %d, resident %d, early form %d" % (le, resident, early_form))


@pytest.mark.parametrize("resident,early_form", [(0, 0), (3, 2)])
def test_option_changed_between_calls(capi, batches, split_levels, reference, resident, early_form):
    got = _sequence(capi, batches, W, H, [0, 2, 0, 3, 1], resident, early_form)
    _same(reference, got, "early levels 0 -> 2 -> 0 -> 3 -> 1, resident %d" % resident)


def test_no_full_cell_is_a_no_op(capi):
    w, h = 160, 120
    assert _full_levels(capi, w, h)[0] == set()
    frames3 = _batches(w, h)
    ref = _sequence(capi, frames3, w, h, 0)
    for early, form in ((1, 0), (50, 2)):
        _same(ref, _sequence(capi, frames3, w, h, early, 0, form), "%dx%d early levels %d" % (w, h, early))
    assert int(ref[0][0][2].min()) > 20


def test_against_the_oracle(capi, oracle, batches, split_levels):
    early, resident, early_form = CASES[0]
    out, _ = _cached((early, resident, early_form), lambda: _sequence(capi, batches, W, H, early, resident, early_form))
    call = CALLS - 1  # (the fifth call: both pairs of buffers have been written by then)
    kp, desc, counts = out[call][:3]
    frames = batches[call % 3]
    for image in (0, 2 * B - 1):
        o = oracle.Orb(nfeatures=NF)
        o.run(frames[image // 2, image & 1])
        rk, rd = o.result()
        n = int(counts[image])
        assert n == len(rk) > 50, "image %d: %d vs %d keypoints" % (image, n, len(rk))
        assert kp[image, :n].tobytes() == rk.tobytes(), "image %d keypoints" % image
        np.testing.assert_array_equal(desc[image, :n], rd, err_msg="image %d descriptors" % image)
