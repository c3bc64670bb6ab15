"""Detection masks (cv::ORB::detectAndCompute's mask argument; include/vsf.h "Detection masks") on the GPU, bit for bit against
tests/orb_mask_ref.py -- keypoints as raw bytes, descriptors and counts per level, no tolerance anywhere.
(tests/test_orb_mask_ref.py pins that reference on the CPU and checks that the scenes used here exercise the feature.)

1. vsf_debug_mask_level equals the reference pyramid as zero / non-zero per pixel at every level, for ten masks, at 160x120 and
   97x75 (8 levels at 1.2) and 640x480 (the reference's 50 levels); from an odd base address and pitch, and from device memory;
2. extraction through vsf_extract, vsf_extract_pair with a different mask per eye and vsf_extract_batch_dev at 1 / 3 / 9 images,
   in HARRIS and FAST_SCORE mode;
3. the FAST forms one at a time at 640x480 (full cells and packed items): one launch for both, two launches, resident with 2 and
   3 waves per SIMD, and pipelined calls on an input event whose early part runs as a grid and resident;
4. levels whose candidates start in HBM (dense_texture) and levels that stay in raster order (line_art within its budget);
5. the killers: all 0, all 254, all 255, after vsf_mask_clear, a slot that other images of the batch do not name;
6. vsf_fast_detect with a mask: any non-zero value passes;
7. refusals leave the slot as it was."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import adversarial_images as adv  # noqa: E402
import orb_mask_ref as ref  # noqa: E402
from oracle import binding as ob  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POISON = 0xA5
SCENES = ref.scenes()
REF_KEYS = ("scale_factor", "nlevels", "edge_threshold", "fast_threshold")


@pytest.fixture(scope="module")
def capi():
    from vision_slam_frontend_amd import capi
    capi.lib()
    return capi


def _params(capi, w, h, n_images, nfeatures, mode, **kw):
    return capi.default_params(w, h, max_images=n_images, nfeatures=nfeatures, score_type=mode, **kw)


def _want(img, mask, nfeatures, mode, kw):
    return ref.reference(img, mask, nfeatures, mode, **{k: v for k, v in kw.items() if k in REF_KEYS})


def _same(kp, desc, want, what):
    rk, rd = want[0], want[1]
    assert len(kp) == len(rk), "%s: %d keypoints, reference %d" % (what, len(kp), len(rk))
    got = np.ascontiguousarray(kp).view(np.uint8).reshape(-1, 28)
    exp = np.ascontiguousarray(rk).view(np.uint8).reshape(-1, 28)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, "%s: keypoint %d of %d differs: %s, reference %s" % (what, bad[0], len(rk), kp[bad[0]], rk[bad[0]])
    bad = np.nonzero((np.asarray(desc) != rd).any(axis=1))[0]
    assert len(bad) == 0, "%s: descriptor %d of %d differs (keypoint %s)" % (what, bad[0], len(rk), rk[bad[0]])


def _level_counts(kp, nlevels):
    return np.bincount(kp["octave"], minlength=nlevels).tolist() if len(kp) else [0] * nlevels


def _packed(imgs, w, h):
    pitch = (w + 15) // 16 * 16
    padded = np.full((len(imgs), h, pitch), 0xFF, np.uint8)
    padded[:, :, :w] = np.stack(imgs)
    return padded, pitch


def _outputs(n, K, dev):
    kp = torch.full((n, K, 28), POISON, dtype=torch.uint8, device=dev)
    de = torch.full((n, K, 32), POISON, dtype=torch.uint8, device=dev)
    cn = torch.full((n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    return kp, de, cn


def _batch(ctx, imgs, w, h):
    dev = torch.device("cuda", 0)
    padded, pitch = _packed(imgs, w, h)
    d = torch.from_numpy(padded).to(dev)
    out = _outputs(len(imgs), ctx.params.max_keypoints, dev)
    ctx.extract_batch_dev(d.data_ptr(), len(imgs), pitch * h, pitch, *[t.data_ptr() for t in out])
    return out


def _check_batch(out, wants, what, capi, nlevels):
    kph, deh, cnh = [t.cpu().numpy() for t in out]
    for i, want in enumerate(wants):
        m = len(want[0])
        assert int(cnh[i]) == m, "%s: image %d has %d keypoints, reference %d" % (what, i, int(cnh[i]), m)
        kp = kph[i, :m].reshape(-1).view(capi.KEYPOINT_DTYPE)
        _same(kp, deh[i, :m], want, "%s image %d" % (what, i))
        assert _level_counts(kp, nlevels) == list(want[2]), "%s image %d: counts per level" % (what, i)
        assert (kph[i, m:] == POISON).all() and (deh[i, m:] == POISON).all(), "%s: image %d written behind row %d" % (what, i, m)


# ---- 1 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,kw", [((160, 120), ref.SMALL), ((97, 75), ref.SMALL), ((640, 480), dict())])
def test_mask_pyramid_equals_the_reference(capi, size, kw):
    w, h = size
    masks = ref.masks(w, h)
    with capi.Context(_params(capi, w, h, 2, 200, ref.HARRIS, **kw)) as ctx:
        sizes = [ctx.level_info(level)[:2] for level in range(ctx.nlevels)]
        assert ctx.mask_slot_bytes() >= sum(sw * sh for sw, sh in sizes)
        dev = torch.device("cuda", 0)
        for slot, (name, mask) in enumerate(sorted(masks.items())):
            want = ref.mask_pyramid(mask, sizes)
            # an odd base address and pitch, from host memory
            pitch = w + 3
            buf = np.full(h * pitch + 8, 0x5A, np.uint8)
            view = buf[1:1 + h * pitch].reshape(h, pitch)[:, :w]
            view[:] = mask
            assert view.ctypes.data % 2 == 1 and view.strides == (pitch, 1)
            ctx.mask_set(slot, view)
            # ... and the same from device memory, into another slot
            d = torch.from_numpy(buf).to(dev)
            torch.cuda.synchronize()
            ctx.mask_set_dev(capi.MAX_MASKS - 1, d.data_ptr() + 1, w, h, pitch)
            assert ctx.mask_is_set(slot) and ctx.mask_is_set(capi.MAX_MASKS - 1)
            for level in range(ctx.nlevels):
                exp = want[level] != 0
                for s in (slot, capi.MAX_MASKS - 1):
                    got = ctx.debug_mask_level(s, level) != 0
                    assert np.array_equal(got, exp), "%s level %d slot %d: %d pixels differ" % (name, level, s, int((got != exp).sum()))


# ---- 2 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [ref.HARRIS, ref.FAST_SCORE])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_extraction_equals_the_reference(capi, name, mode):
    img, mask, nfeatures, kw = SCENES[name]
    h, w = img.shape
    other_img = np.ascontiguousarray(img[::-1, ::-1])
    other_mask = np.ascontiguousarray(mask[::-1, ::-1])  # the other eye sees another housing
    assert other_mask.tobytes() != mask.tobytes()
    want_a, want_b = _want(img, mask, nfeatures, mode, kw), _want(other_img, other_mask, nfeatures, mode, kw)
    want_ab, want_ba = _want(img, other_mask, nfeatures, mode, kw), _want(other_img, mask, nfeatures, mode, kw)
    plain = _want(img, None, nfeatures, mode, kw)
    assert want_a[0].tobytes() != plain[0].tobytes()
    big = w >= 640
    with capi.Context(_params(capi, w, h, 3 if big else 9, nfeatures, mode, max_keypoints=nfeatures + 512, **kw)) as ctx:
        nl = ctx.nlevels
        assert ctx.get_image_masks() == (-1, -1)
        ctx.mask_set(5, mask)
        ctx.mask_set(40, other_mask)
        _same(*ctx.extract(img), plain, name + " vsf_extract before vsf_set_image_masks")
        ctx.set_image_masks(5, 40)
        assert ctx.get_image_masks() == (5, 40)
        kp, desc = ctx.extract(img)
        _same(kp, desc, want_a, name + " vsf_extract")
        assert _level_counts(kp, nl) == list(want_a[2])
        (k0, d0), (k1, d1) = ctx.extract_pair(img, other_img)
        _same(k0, d0, want_a, name + " vsf_extract_pair left")
        _same(k1, d1, want_b, name + " vsf_extract_pair right")
        for n in ((3,) if big else (1, 3, 9)):
            imgs = [img if (i % 3) != 1 else other_img for i in range(n)]  # (image and slot alternate at different periods)
            wants = []
            for i in range(n):
                first = (i % 3) != 1
                wants.append((want_a if first else want_ba) if i % 2 == 0 else (want_ab if first else want_b))
            out = _batch(ctx, imgs, w, h)
            assert ctx.sync() == capi.VSF_OK
            _check_batch(out, wants, "%s batch of %d" % (name, n), capi, nl)


# ---- 3 ----------------------------------------------------------------------------------------------------------------

def _forms_scene():
    img, mask, nfeatures, kw = SCENES["synth640_disc"]
    m2 = ref.masks(640, 480)["rectangle_two_borders"]
    imgs = [img, np.ascontiguousarray(img[:, ::-1]), np.ascontiguousarray(img[::-1, :])]
    return imgs, (mask, m2), nfeatures, kw


@pytest.mark.parametrize("form", ["both", "two_launches", "resident2", "resident3"])
def test_fast_forms(capi, form):
    imgs, (ma, mb), nfeatures, kw = _forms_scene()
    wants = [_want(im, ma if i % 2 == 0 else mb, nfeatures, ref.HARRIS, kw) for i, im in enumerate(imgs)]
    with capi.Context(_params(capi, 640, 480, 3, nfeatures, ref.HARRIS)) as ctx:
        if form == "two_launches":
            ctx.set_option(capi.OPT_FAST_BOTH_MAX, 0)
        elif form.startswith("resident"):
            ctx.set_fast_resident(int(form[-1]))
        ctx.mask_set(0, ma)
        ctx.mask_set(1, mb)
        ctx.set_image_masks(0, 1)
        out = _batch(ctx, imgs, 640, 480)
        assert ctx.sync() == capi.VSF_OK
        _check_batch(out, wants, "form " + form, capi, ctx.nlevels)


@pytest.mark.parametrize("early_form", [0, 2])
def test_pipelined_calls_with_an_input_event(capi, early_form):
    imgs, (ma, mb), nfeatures, kw = _forms_scene()
    w, h, N = 640, 480, 4
    order = [[0, 1, 2, 0], [2, 0, 1, 1]]
    dev = torch.device("cuda", 0)
    wants = [[_want(imgs[j], ma if i % 2 == 0 else mb, nfeatures, ref.HARRIS, kw) for i, j in enumerate(o)] for o in order]
    with capi.Context(_params(capi, w, h, N, nfeatures, ref.HARRIS)) as ctx:
        ctx.mask_set(2, ma)
        ctx.mask_set(3, mb)
        ctx.set_image_masks(2, 3)
        ctx.set_pipeline(True)
        ctx.set_option(capi.OPT_FAST_EARLY_LEVELS, 2)
        ctx.set_option(capi.OPT_FAST_EARLY_FORM, early_form)
        K = ctx.params.max_keypoints
        staged, d_img = [], []
        for o in order:
            padded, pitch = _packed([imgs[j] for j in o], w, h)
            staged.append(torch.from_numpy(padded).pin_memory())
            d_img.append(torch.zeros(padded.shape, dtype=torch.uint8, device=dev))
        outs = [_outputs(N, K, dev) for _ in range(3)]
        producer = torch.cuda.Stream(device=dev)
        ready = [torch.cuda.Event() for _ in range(3)]
        for c in range(3):
            b = c & 1
            if c == 2:
                ctx.sync()  # (buffer 0 is written again: call 0 has read it by now)
                d_img[b].zero_()
                torch.cuda.synchronize()
            with torch.cuda.stream(producer):
                d_img[b].copy_(staged[b], non_blocking=True)
                ready[c].record(producer)
            ctx.set_input_event(ready[c].cuda_event)
            ctx.extract_batch_dev(d_img[b].data_ptr(), N, pitch * h, pitch, *[t.data_ptr() for t in outs[c]])
        assert ctx.sync() == capi.VSF_OK
        torch.cuda.synchronize()
        for c in range(3):
            _check_batch(outs[c], wants[c & 1], "pipelined call %d, early form %d" % (c, early_form), capi, ctx.nlevels)


# ---- 4 ----------------------------------------------------------------------------------------------------------------

def test_levels_in_hbm_and_levels_in_raster_order(capi):
    m = ref.masks(640, 480)
    dense, line = adv.dense_texture(), adv.line_art()
    orb = ref.run_oracle(dense, 2000)
    kept = ref.filter_by_mask(orb.stage(0, 0), m["rectangle_two_borders"])
    assert len(kept) > 12288 and len(kept) < len(orb.stage(0, 0))  # behind the filter still above every LDS array: stage 1 in HBM
    want_dense = _want(dense, m["rectangle_two_borders"], 2000, ref.HARRIS, {})
    with capi.Context(_params(capi, 640, 480, 3, 2000, ref.HARRIS)) as ctx:
        ctx.mask_set(0, m["rectangle_two_borders"])
        ctx.set_image_masks(0, 0)
        _same(*ctx.extract(dense), want_dense, "dense_texture vsf_extract")
        flat = np.full((480, 640), 17, np.uint8)
        out = _batch(ctx, [flat, dense, dense], 640, 480)
        assert ctx.sync() == capi.VSF_OK
        empty = (np.zeros(0, capi.KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), [0] * ctx.nlevels)
        _check_batch(out, [empty, want_dense, want_dense], "flat | dense | dense", capi, ctx.nlevels)
    # line_art at nfeatures 10000: level 0 and levels 20 .. 37 stay within n_l, where the lists keep raster order
    orb = ref.run_oracle(line, 10000)
    pyr = ref.mask_pyramid(m["disc"], ref.level_sizes(orb))
    within = [l for l in range(orb.nlevels) if 0 < len(ref.filter_by_mask(orb.stage(0, l), pyr[l])) <= orb.level_info(l)[3]]
    assert len(within) >= 10, within
    want_line = _want(line, m["disc"], 10000, ref.FAST_SCORE, {})
    with capi.Context(_params(capi, 640, 480, 1, 10000, ref.FAST_SCORE)) as ctx:
        ctx.mask_set(7, m["disc"])
        ctx.set_image_masks(7, -1)
        _same(*ctx.extract(line), want_line, "line_art vsf_extract")


# ---- 5 ----------------------------------------------------------------------------------------------------------------

def test_killers(capi):
    img, mask, nfeatures, kw = SCENES["noise160_half"]
    h, w = img.shape
    m = ref.masks(w, h)
    plain = _want(img, None, nfeatures, ref.HARRIS, kw)
    with capi.Context(_params(capi, w, h, 4, nfeatures, ref.HARRIS, **kw)) as ctx:
        K = ctx.params.max_keypoints
        ctx.set_image_masks(0, 0)
        _same(*ctx.extract(img), plain, "a slot that was never set")
        # all 0: VSF_OK, zero keypoints, nothing written
        ctx.mask_set(0, m["all0"])
        kp = np.full(K * 28, POISON, np.uint8)
        desc = np.full((K, 32), POISON, np.uint8)
        n = C.c_int(-1)
        st = capi.lib().vsf_extract(ctx._h, img.ctypes.data_as(C.c_void_p), w, h, w, kp.ctypes.data_as(C.c_void_p),
                                    desc.ctypes.data_as(C.c_void_p), K, C.byref(n))
        assert st == capi.VSF_OK and n.value == 0
        assert (kp == POISON).all() and (desc == POISON).all()
        # all 254: level-0 keypoints only
        ctx.mask_set(0, m["all254"])
        want254 = _want(img, m["all254"], nfeatures, ref.HARRIS, kw)
        assert want254[2][0] == plain[2][0] > 0 and sum(want254[2][1:]) == 0
        kp254, d254 = ctx.extract(img)
        _same(kp254, d254, want254, "all 254")
        assert (kp254["octave"] == 0).all()
        # all 255: byte-identical to the same context with no mask
        ctx.mask_set(0, m["all255"])
        k255, d255 = ctx.extract(img)
        ctx.set_image_masks(-1, -1)
        k0, d0 = ctx.extract(img)
        assert k255.tobytes() == k0.tobytes() == plain[0].tobytes() and np.array_equal(d255, d0)
        # after vsf_mask_clear: no mask
        ctx.mask_set(0, mask)
        ctx.set_image_masks(0, 0)
        _same(*ctx.extract(img), _want(img, mask, nfeatures, ref.HARRIS, kw), "half plane")
        ctx.mask_clear(0)
        assert not ctx.mask_is_set(0)
        _same(*ctx.extract(img), plain, "after vsf_mask_clear")
        # one mixed batch: slot 3 masks the even images; the odd ones name slot 9, which holds no mask, resp. none at all
        ctx.mask_set(3, mask)
        masked = _want(img, mask, nfeatures, ref.HARRIS, kw)
        for odd in (9, -1):
            ctx.set_image_masks(3, odd)
            out = _batch(ctx, [img] * 4, w, h)
            assert ctx.sync() == capi.VSF_OK
            _check_batch(out, [masked, plain, masked, plain], "slot 3 | slot %d" % odd, capi, ctx.nlevels)
        ctx.set_image_masks(-1, 3)
        out = _batch(ctx, [img] * 3, w, h)
        assert ctx.sync() == capi.VSF_OK
        _check_batch(out, [plain, masked, plain], "none | slot 3", capi, ctx.nlevels)


# ---- 6 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nms", [True, False])
def test_fast_detect_with_a_mask(capi, nms):
    w, h = 160, 120
    img = ref._noise(w, h, 11)
    mask = ref.masks(w, h)["stripes_1_128_254_255"].copy()
    mask[:, 100:] = 0
    mask[40:60, :] = 0
    full = ob.fast9_16(img, 25, nms)
    keep = mask[full["y"].astype(np.int64), full["x"].astype(np.int64)] != 0
    assert 0 < keep.sum() < len(full)
    with capi.Context(_params(capi, w, h, 1, 100, ref.HARRIS, **ref.SMALL)) as ctx:
        assert ctx.fast_detect(img, 25, nms).tobytes() == full.tobytes()
        ctx.mask_set(1, mask)
        ctx.set_image_masks(1, -1)
        assert ctx.fast_detect(img, 25, nms).tobytes() == full[keep].tobytes()
        ctx.set_image_masks(-1, 1)  # (the one image of the call is image 0: even)
        assert ctx.fast_detect(img, 25, nms).tobytes() == full.tobytes()


# ---- 7 ----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_slot_as_it_was(capi):
    w, h = 160, 120
    m = ref.masks(w, h)
    L = capi.lib()
    inv = capi.VSF_ERR_INVALID_ARG
    with capi.Context(_params(capi, w, h, 1, 100, ref.HARRIS, **ref.SMALL)) as ctx:
        ctx.mask_set(2, m["disc"])
        before = [ctx.debug_mask_level(2, level) for level in range(ctx.nlevels)]
        p = m["all0"].ctypes.data_as(C.c_void_p)
        assert L.vsf_mask_set(ctx._h, 2, p, w - 1, h, w) == inv          # another size
        assert L.vsf_mask_set(ctx._h, 2, p, w, h + 1, w) == inv
        assert L.vsf_mask_set(ctx._h, 2, p, w, h, w - 1) == inv          # rows overlap
        assert L.vsf_mask_set(ctx._h, 2, None, w, h, w) == inv           # null pointer
        assert L.vsf_mask_set_dev(ctx._h, 2, None, w, h, w) == inv
        for bad in (-1, capi.MAX_MASKS, 1 << 20):
            assert L.vsf_mask_set(ctx._h, bad, p, w, h, w) == inv        # bad slot
            assert L.vsf_mask_clear(ctx._h, bad) == inv
        assert L.vsf_set_image_masks(ctx._h, -2, 0) == inv and L.vsf_set_image_masks(ctx._h, 0, capi.MAX_MASKS) == inv
        assert ctx.get_image_masks() == (-1, -1)
        assert L.vsf_debug_mask_level(ctx._h, 3, 0, p, w) == inv         # a slot that holds no mask
        assert ctx.mask_is_set(2)
        for level, want in enumerate(before):
            assert np.array_equal(ctx.debug_mask_level(2, level), want)
