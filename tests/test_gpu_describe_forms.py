"""Both instantiations of orb_orient_describe_kernel (four and eight consecutive output keypoints per wave) against the
oracle, each chosen by the real dispatch: the tests ask vsf_debug_describe_form which form a batch takes instead of
restating the launcher's thresholds, run batches on either side of the change, and hold every image's counts, keypoints
and descriptors against the oracle byte for byte.  (The benchmark's --nfeatures 10000 row, 512 images x 10 256 keypoints,
runs the eight-per-wave form.)

320x240 images, the default 50 x 1.04 pyramid, nfeatures = 10000.  The 16 distinct images, repeated cyclically to fill a
batch (oracle totals in brackets): a flat image (0); one bright square (120); (left, right) stereo pairs of
400, 120, 60, 30, 12 and 5 objects (6133 / 6204, 3769 / 3822, 2575 / 2681, 1242 / 955, 102 / 217, 0 / 4); the left image
of a 4-object scene (85, groups of eight spanning 7 levels); uniform noise (4704).  Pairs sit at (even, odd) indices, so
frame f of a stereo batch is pair f mod 8."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, H, NF = 320, 240, 10000
POISON = 0xA5


@pytest.fixture(scope="module")
def capi():
    from vision_slam_frontend_amd import capi
    capi.lib()
    return capi


def _image_set():
    from vision_slam_frontend_amd import synth
    flat = np.full((H, W), 97, np.uint8)
    square = np.full((H, W), 60, np.uint8)
    square[100:140, 150:200] = 200
    imgs = [flat, square]
    for n_objects in (400, 120, 60, 30, 12, 5):
        imgs += list(synth.stereo_pair(W, H, 3, n_objects=n_objects))
    imgs.append(synth.stereo_pair(W, H, 3, n_objects=4)[0])
    imgs.append(np.random.default_rng(5).integers(0, 256, (H, W), dtype=np.uint8))
    assert len(imgs) == 16
    return np.stack([np.ascontiguousarray(i, np.uint8) for i in imgs])


@pytest.fixture(scope="module")
def refs(oracle):
    """(images, [(keypoints, descriptors)] of the oracle, one run per distinct image); shared, never modified."""
    imgs = _image_set()
    out = []
    for img in imgs:
        o = oracle.Orb(nfeatures=NF)
        o.run(img)
        out.append(o.result())
    return imgs, out


def _assert_input_conditions(refs, K):
    """What makes the image set worth running, from the oracle's results alone."""
    totals = [len(rk) for rk, _ in refs[1]]
    assert 0 in totals, totals
    assert any(1 <= t <= 7 or (t < K and t % 8) for t in totals), totals  # a last wave of fewer than eight
    assert sum(t > K for t in totals) >= 2, totals
    below = [t for t in totals if t < K]
    assert len(below) >= 4, totals
    assert len({t % 8 for t in below}) >= 4, totals
    spans = 0
    for rk, _ in refs[1]:
        octv = rk["octave"][:min(len(rk), K)]
        spans = max([spans] + [len(set(octv[g:g + 8].tolist())) for g in range(0, len(octv), 8)])
    assert spans >= 3, "no aligned group of eight output keypoints spans three octaves (%d)" % spans


def _first_form8(ctx, candidates):
    return next((n for n in candidates if ctx.debug_describe_form(n) == 8), None)


def _ref_tensors(refs, dev):
    out = []
    for rk, rd in refs[1]:
        kb = np.ascontiguousarray(rk).view(np.uint8).reshape(-1, 28)
        out.append((torch.from_numpy(kb.copy()).to(dev), torch.from_numpy(np.ascontiguousarray(rd).copy()).to(dev)))
    return out


def _check_against_oracle(refs, ref_dev, kp, de, cn, n, K, what):
    """Images [0, n) of the device buffers (image i shows distinct image i mod 16): counts, the first min(count, K) records
    equal to the oracle's, every row behind them untouched.  Compared on the device, one distinct image at a time."""
    counts = cn.cpu().numpy()
    for j, (rk, _) in enumerate(refs[1]):
        idx = torch.arange(j, n, 16, device=kp.device)
        if len(idx) == 0:
            continue
        total, m = len(rk), min(len(rk), K)
        assert (counts[j:n:16] == total).all(), "%s: counts of image %d mod 16: %s, oracle %d" % (what, j, counts[j:n:16], total)
        for name, got, want in (("keypoints", kp, ref_dev[j][0]), ("descriptors", de, ref_dev[j][1])):
            rows = got[idx]
            if m:
                bad = (rows[:, :m] != want[None, :m]).any(dim=2).nonzero()
                assert len(bad) == 0, "%s: %s of image %d, row %d differ from the oracle (%d of %d rows)" % (
                    what, name, j + 16 * int(bad[0, 0]), int(bad[0, 1]), len(bad), m * len(idx))
            assert bool((rows[:, m:] == POISON).all()), "%s: %s of image %d mod 16 written at or behind row %d" % (what, name, j, m)
    if n < kp.shape[0]:
        assert bool((kp[n:] == POISON).all()) and bool((de[n:] == POISON).all()), "%s: images behind the batch written" % what
        assert (counts[n:] == -1).all()


def test_query(capi):
    """vsf_debug_describe_form: 4 below either threshold, 8 for the benchmark's nfeatures = 10000 shape, an error for no
    context or no images."""
    L = capi.lib()
    assert L.vsf_debug_describe_form(None, 512) == capi.VSF_ERR_INVALID_ARG
    with capi.Context(capi.default_params(W, H, max_images=2, nfeatures=NF, max_keypoints=4095)) as ctx:
        assert ctx.params.max_keypoints == 4095
        assert [ctx.debug_describe_form(n) for n in (1, 2, 731, 732, 733, 1 << 20)] == [4] * 6
        assert L.vsf_debug_describe_form(ctx._h, 0) == capi.VSF_ERR_INVALID_ARG
        with pytest.raises(capi.VsfError):
            ctx.debug_describe_form(-3)
    with capi.Context(capi.default_params(W, H, max_images=2, nfeatures=NF)) as ctx:
        assert ctx.params.max_keypoints == NF + 256
        assert ctx.debug_describe_form(2) == 4
        assert ctx.debug_describe_form(256) == 4   # the largest batch the ObserveImage queue hands over
        assert ctx.debug_describe_form(512) == 8   # bench.py --nfeatures 10000
    # ... and at the two shapes the tests below run (found by the query, so this only says that there is such a shape)
    for K, cand in ((4100, range(1, 1025)), (65535, range(2, 129, 2))):
        with capi.Context(capi.default_params(W, H, max_images=2, nfeatures=NF, max_keypoints=K)) as ctx:
            n8 = _first_form8(ctx, cand)
            assert n8 is not None and ctx.debug_describe_form(n8) == 8 and ctx.debug_describe_form(1) == 4


def test_dispatch_edge_with_truncation(capi, refs):
    """max_keypoints = 4100 (>= 4096, no multiple of 8: a truncated image ends in a wave of four): n8 - 1 images run the
    four-per-wave form, n8 images the eight-per-wave form, n8 the smallest batch for which the query says 8."""
    K = 4100
    _assert_input_conditions(refs, K)
    dev = torch.device("cuda", 0)
    with capi.Context(capi.default_params(W, H, max_images=2, nfeatures=NF, max_keypoints=K)) as probe:
        n8 = _first_form8(probe, range(1, 1025))
    assert n8 is not None and n8 >= 2, "no batch of up to 1024 images takes the eight-per-wave form"
    print("n8 at max_keypoints = %d: %d" % (K, n8))
    ref_dev = _ref_tensors(refs, dev)
    with capi.Context(capi.default_params(W, H, max_images=n8, nfeatures=NF, max_keypoints=K)) as ctx:
        assert ctx.params.max_keypoints == K
        d_img = torch.from_numpy(refs[0]).to(dev)[torch.arange(n8, device=dev) % 16].contiguous()
        kp = torch.empty((n8, K, 28), dtype=torch.uint8, device=dev)
        de = torch.empty((n8, K, 32), dtype=torch.uint8, device=dev)
        cn = torch.empty(n8, dtype=torch.int32, device=dev)
        for n, form in ((n8 - 1, 4), (n8, 8)):
            assert ctx.debug_describe_form(n) == form
            kp.fill_(POISON)
            de.fill_(POISON)
            cn.fill_(-1)
            torch.cuda.synchronize()
            ctx.extract_batch_dev(d_img.data_ptr(), n, W * H, W, kp.data_ptr(), de.data_ptr(), cn.data_ptr())
            assert ctx.sync(allow_capacity=True) == capi.VSF_ERR_CAPACITY  # some images overflow
            _check_against_oracle(refs, ref_dev, kp, de, cn, n, K, "%d images, %d keypoints per wave" % (n, form))


def test_stereo_step_under_form8_with_few_images(capi, oracle, refs):
    """max_keypoints = 65535: a few dozen images are enough for the eight-per-wave form, so the whole stereo step (extract
    and matcher) runs it with nothing truncated; the same frames through a context that takes four per wave give the same
    bytes."""
    K = 65535
    dev = torch.device("cuda", 0)
    with capi.Context(capi.default_params(W, H, max_images=2, nfeatures=NF, max_keypoints=K)) as probe:
        n = _first_form8(probe, range(2, 129, 2))
    assert n is not None, "no even batch of up to 128 images takes the eight-per-wave form"
    print("smallest even batch under form 8 at max_keypoints = %d: %d" % (K, n))
    B = n // 2
    ref_dev = _ref_tensors(refs, dev)
    ref_matches = [oracle.get_matches(refs[1][2 * f][1], refs[1][2 * f + 1][1]) for f in range(8)]
    assert sum(len(m) for m in ref_matches) > 100

    def buffers(nf):
        b = (torch.empty((2 * nf, K, 28), dtype=torch.uint8, device=dev), torch.empty((2 * nf, K, 32), dtype=torch.uint8, device=dev),
             torch.empty(2 * nf, dtype=torch.int32, device=dev), torch.empty((nf, K, 16), dtype=torch.uint8, device=dev),
             torch.empty(nf, dtype=torch.int32, device=dev))
        for t in b:
            t.fill_(POISON if t.dtype == torch.uint8 else -1)
        return b

    base = torch.from_numpy(refs[0]).to(dev)
    with capi.Context(capi.default_params(W, H, max_images=n, nfeatures=NF, max_keypoints=K)) as ctx:
        assert ctx.debug_describe_form(n) == 8
        d_img = base[torch.arange(n, device=dev) % 16].contiguous()
        kp, de, cn, dm, nm = buffers(B)
        torch.cuda.synchronize()
        ctx.stereo_batch_dev(d_img.data_ptr(), B, W * H, W, kp.data_ptr(), de.data_ptr(), cn.data_ptr(), dm.data_ptr(), nm.data_ptr())
        assert ctx.sync() == capi.VSF_OK
        _check_against_oracle(refs, ref_dev, kp, de, cn, n, K, "stereo step, %d images, 8 keypoints per wave" % n)
        nmh = nm.cpu().numpy()
        for f in range(B):
            rm = ref_matches[f % 8]
            assert int(nmh[f]) == len(rm), "frame %d: %d matches, oracle %d" % (f, int(nmh[f]), len(rm))
            assert dm[f, :len(rm)].cpu().numpy().tobytes() == rm.tobytes(), "frame %d matches" % f
    # the eight distinct frames, two at a time, where the query says 4
    with capi.Context(capi.default_params(W, H, max_images=4, nfeatures=NF, max_keypoints=K)) as ctx:
        assert ctx.debug_describe_form(4) == 4
        small = buffers(8)
        torch.cuda.synchronize()
        for f0 in range(0, 8, 2):
            ctx.stereo_batch_dev(base[2 * f0:].data_ptr(), 2, W * H, W, small[0][2 * f0:].data_ptr(), small[1][2 * f0:].data_ptr(),
                                 small[2][2 * f0:].data_ptr(), small[3][f0:].data_ptr(), small[4][f0:].data_ptr())
        assert ctx.sync() == capi.VSF_OK
    # (keypoints and descriptors whole, poison behind the counts included; the matcher's rows up to each frame's count)
    for name, big, sm, per in (("keypoints", kp, small[0], 16), ("descriptors", de, small[1], 16), ("counts", cn, small[2], 16),
                               ("match counts", nm, small[4], 8)):
        want = sm[torch.arange(big.shape[0], device=dev) % per]
        assert torch.equal(big, want), "%s: the batch under form 8 differs from the same frames under form 4" % name
    for f in range(B):
        assert torch.equal(dm[f, :int(nmh[f])], small[3][f % 8, :int(nmh[f])]), "matches of frame %d differ between the forms" % f
