"""The reference's debug images (slam_frontend.cc:74-115, 458-495) drawn on the GPU (csrc/k_draw.hip):

- vsf_draw_canvases_dev against the restatement of OpenCV 3.2's Circle / LineIterator / clipLine (tests/draw_ref.py), byte
  for byte, on random operation lists: heavy overlap (draw order decides), clipped and wholly off-canvas primitives, one
  and two source images, batches of 1 and 64 canvases;
- slam::Frontend with debug images on, fused, per call and pipelined (depths 1, 4, 32), against images the restatement
  draws from the oracle model's kept keypoints and sorted matches, with the line colours regenerated from libc's rand()
  after the same srand(seed);
- with the switch off: empty getters, and queue results byte-identical to a context whose switch was never touched."""
import ctypes as C

import numpy as np
import pytest

import draw_ref as D

pytestmark = pytest.mark.gpu

NF = 1000
F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)  # l^T F r = y_r - y_l: rectified synthetic pair
SEED = 4242


def _random_ops(rng, n, w, h):
    ops = []
    for _ in range(n):
        col = tuple(int(v) for v in rng.integers(0, 256, 3))
        kind = int(rng.integers(0, 2))
        if rng.random() < 0.15:  # far outside, partly or wholly
            x0, y0, x1, y1 = (int(v) for v in rng.integers(-3 * w, 4 * w, 4))
        else:  # a small region: heavy overlap
            x0, x1 = (int(v) for v in rng.integers(-8, w + 8, 2))
            y0, y1 = (int(v) for v in rng.integers(-8, h + 8, 2))
        if kind == D.CIRCLE:
            x1, y1 = int(rng.integers(0, 12)), 0
        ops.append((kind, x0, y0, x1, y1, col))
    return ops


def _ops_array(ops):
    from vision_slam_frontend_amd import capi
    a = np.zeros(max(len(ops), 1), capi.DRAW_OP_DTYPE)
    for i, (kind, x0, y0, x1, y1, col) in enumerate(ops):
        a[i] = (kind, x0, y0, x1, y1, (col[0], col[1], col[2], 0))
    return a


@pytest.mark.parametrize("n_canvases", [1, 64])
def test_draw_canvases_dev_matches_restatement(n_canvases):
    import torch
    from vision_slam_frontend_amd import capi
    rng = np.random.default_rng(n_canvases)
    w, h = 48, 36
    dev = torch.device("cuda:0")
    srcs, canvases, all_ops, want = [], [], [], []
    for c in range(n_canvases):
        two = bool(c % 2) or n_canvases == 1
        g0 = rng.integers(0, 256, (h, w), dtype=np.uint8)
        g1 = rng.integers(0, 256, (h, w), dtype=np.uint8) if two else None
        ops = _random_ops(rng, int(rng.integers(0, 120)), w * (2 if two else 1), h)
        want.append(D.render(g0, g1, ops))
        t0 = torch.from_numpy(g0).to(dev)
        t1 = torch.from_numpy(g1).to(dev) if two else None
        out = torch.zeros((h, w * (2 if two else 1), 3), dtype=torch.uint8, device=dev)
        srcs.append((t0, t1, out))
        canvases.append({"src0": t0.data_ptr(), "src1": t1.data_ptr() if two else None, "width": w, "height": h,
                         "src_pitch": w, "out": out.data_ptr(), "out_pitch": out.shape[1] * 3,
                         "op_begin": len(all_ops), "op_count": len(ops)})
        all_ops += ops
    d_ops = torch.from_numpy(_ops_array(all_ops).view(np.uint8)).to(dev)
    torch.cuda.synchronize()
    with capi.Context(capi.default_params(64, 64, max_images=2, nfeatures=100), device=0) as ctx:
        for _ in range(2):  # twice: the winner buffer must be clean again after the first call
            for _, _, out in srcs:
                out.zero_()
            torch.cuda.synchronize()
            ctx.draw_canvases_dev(canvases, d_ops.data_ptr(), len(all_ops))
            assert ctx.sync() == capi.VSF_OK
            for c, (_, _, out) in enumerate(srcs):
                got = out.cpu().numpy()
                assert np.array_equal(got, want[c]), "canvas %d: %d bytes differ" % (c, int((got != want[c]).sum()))


def _libc():
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    libc.srand.argtypes = [C.c_uint]
    return libc


def _sequence():
    from vision_slam_frontend_amd import synth
    sc = synth.Scene(640, 480)
    frames = [(sc.render(f, 0), sc.render(f, 1)) for f in range(7)]
    # frame 3 has an empty right image: no stereo match (cc:131-133, no stereo image), and its NaN threshold leaves frame 4
    # with nothing either (quirk Q3); frame 5 is filtered normally again
    frames[3] = (frames[3][0], np.zeros_like(frames[3][1]))
    return frames


def _expected(oracle, frames, frame_life, best_percent=np.float32(0.3)):
    """The oracle model of ObserveImage (as in test_gpu_frontend.py) with what the debug images are drawn from:
    per node (stereo ops or None, their colour count, match ops or None)."""
    thr = np.float32(10000.0)
    frame_list, out = [], []
    for fid, (left, right) in enumerate(frames):
        ol, orr = oracle.Orb(nfeatures=NF), oracle.Orb(nfeatures=NF)
        ol.run(left)
        orr.run(right)
        kl, dl = ol.result()
        kr, dr = orr.result()
        m = oracle.get_matches(dl, dr)
        keep, _, thr_new, _ = oracle.remove_ambig_stereo(kl, kr, m, F_RECT, float(thr))
        thr = np.float32(thr_new)
        kl2, dl2 = kl[m["queryIdx"][keep]], dl[m["queryIdx"][keep]]
        kr2, dr2 = kr[m["trainIdx"][keep]], dr[m["trainIdx"][keep]]
        factors = []
        for pid, pk, pd in frame_list:
            mm = oracle.sort_and_trim(oracle.get_matches(pd, dl2), float(best_percent))
            factors.append((pk, np.stack([mm["queryIdx"], mm["trainIdx"]], 1)))
        st = oracle.sort_and_trim(oracle.get_matches(dr2, dl2), 1.0)  # Calculate3DPoints: right -> left, all of them
        stereo = np.stack([st["queryIdx"], st["trainIdx"]], 1) if len(st) else None
        match = None
        if frame_list:  # cc:458-466: against frame_list_.back(), the newest kept frame
            pk, pairs = factors[-1]
            match = D.match_ops(pk, kl2, pairs)
        out.append((left, right, kl2, kr2, stereo, match))
        if len(frame_list) >= frame_life:
            frame_list.pop(0)
        frame_list.append((fid, kl2, dl2))
    return out


def _draw_expected(model, libc):
    libc.srand(SEED)
    stereo_imgs, match_imgs = [], []
    for left, right, kl2, kr2, stereo, match in model:
        if stereo is not None:
            cols = D.rand_colours(libc.rand, len(stereo))
            stereo_imgs.append(D.render(left, right, D.stereo_ops(kl2, kr2, stereo, left.shape[1], cols)))
        if match is not None:
            match_imgs.append(D.render(left, None, match))
    return stereo_imgs, match_imgs


MODES = [("fused", None), ("per_call", None), ("pipelined", 1), ("pipelined", 4), ("pipelined", 32)]


@pytest.fixture(scope="module")
def expected_images(oracle):
    frames = _sequence()
    model = _expected(oracle, frames, frame_life=3)
    stereo_imgs, match_imgs = _draw_expected(model, _libc())
    return frames, model, stereo_imgs, match_imgs


@pytest.mark.parametrize("mode,depth", MODES)
def test_frontend_debug_images_match_reference(expected_images, mode, depth):
    from vision_slam_frontend_amd import frontend
    frames, model, stereo_imgs, match_imgs = expected_images
    # the model's shape: the empty right image gives two nodes without a stereo image, the first node has no match image
    assert model[3][4] is None and model[4][4] is None and all(m[4] is not None for i, m in enumerate(model) if i not in (3, 4))
    assert len(stereo_imgs) == len(frames) - 2 and len(match_imgs) == len(frames) - 1
    libc = _libc()
    libc.srand(SEED)
    fe = frontend.Frontend(640, 480, nfeatures=NF, fundamental=F_RECT, frame_life=3, debug_images=True)
    if mode == "per_call":
        fe.set_fused(False)
    if mode == "pipelined":
        fe.set_pipelined(True)
        fe.set_queue(depth=depth)
    q = np.array([1, 0, 0, 0], np.float32)
    fe.observe_odometry([0, 0, 0], q, 1.0)
    assert fe.last_debug_image() is None and fe.last_debug_image(stereo=True) is None
    for f, (left, right) in enumerate(frames):
        fe.observe_odometry([0.3 * (f + 1), 0, 0], q, 10.0 + f)
        assert fe.observe_image(left, right) is True
    got_stereo, got_match = fe.debug_images(stereo=True), fe.debug_images()
    assert fe.num_poses == len(frames)
    assert len(got_stereo) == len(stereo_imgs) and len(got_match) == len(match_imgs)
    for i, (g, w) in enumerate(zip(got_stereo, stereo_imgs)):
        assert g.shape == (480, 1280, 3) and np.array_equal(g, w), "stereo image %d: %d bytes differ" % (i, (g != w).sum())
    for i, (g, w) in enumerate(zip(got_match, match_imgs)):
        assert g.shape == (480, 640, 3) and np.array_equal(g, w), "match image %d: %d bytes differ" % (i, (g != w).sum())
    assert np.array_equal(fe.last_debug_image(stereo=True), stereo_imgs[-1])
    assert np.array_equal(fe.last_debug_image(), match_imgs[-1])
    fe.close()


def test_debug_images_off(oracle):
    from vision_slam_frontend_amd import capi, frontend, synth
    sc = synth.Scene(320, 240)
    frames = [(sc.render(f, 0), sc.render(f, 1)) for f in range(3)]
    fe = frontend.Frontend(320, 240, nfeatures=500, fundamental=F_RECT, frame_life=3)
    q = np.array([1, 0, 0, 0], np.float32)
    fe.observe_odometry([0, 0, 0], q, 1.0)
    for f, (left, right) in enumerate(frames):
        fe.observe_odometry([0.3 * (f + 1), 0, 0], q, 10.0 + f)
        assert fe.observe_image(left, right) is True
    assert fe.debug_images() == [] and fe.debug_images(stereo=True) == []
    assert fe.last_debug_image() is None and fe.last_debug_image(stereo=True) is None
    fe.close()
    # the queue: a context whose switch went on and off again returns what one that never saw it does, byte for byte;
    # with it on, the same bytes but for header words 14 (images present) and 15 (colours taken), and the images in view
    calib = frontend.default_calibration().set("fundamental", F_RECT.reshape(9))
    L = capi.lib()

    def run(setting):
        with capi.Context(capi.default_params(320, 240, max_images=2, nfeatures=500), device=0) as ctx:
            for v in setting:
                assert L.vsf_observe_set_debug_images(ctx._h, v) == capi.VSF_OK
            cap = L.vsf_observe_capacity(ctx._h, 3)
            outs, views = [], []
            for left, right in frames:
                buf = np.zeros(cap, np.uint8)
                n, t = C.c_size_t(), C.c_int64()
                assert L.vsf_observe_submit(ctx._h, left.ctypes.data, right.ctypes.data, 320, 240, 320, C.byref(calib),
                                            C.c_float(0.3), 3, C.byref(t)) == capi.VSF_OK
                assert L.vsf_observe_collect(ctx._h, t.value, buf.ctypes.data, cap, C.byref(n)) == capi.VSF_OK
                outs.append(buf[:n.value].copy())
                s_, m_ = C.c_void_p(), C.c_void_p()
                views.append(L.vsf_observe_debug_view(ctx._h, t.value, C.byref(s_), C.byref(m_)) == capi.VSF_OK and
                             (bool(s_.value), bool(m_.value)))
            # the window holds frames: the switch no longer moves
            assert L.vsf_observe_set_debug_images(ctx._h, 0 if 1 in setting[-1:] else 1) == capi.VSF_ERR_INVALID_ARG
            return cap, outs, views

    cap0, plain, v0 = run([])
    cap1, toggled, _ = run([1, 0])
    cap2, on, v2 = run([1])
    assert cap1 == cap0 == cap2 and v0 == [False] * len(frames)
    assert v2 == [(True, False)] + [(True, True)] * (len(frames) - 1)
    for a, b, c in zip(plain, toggled, on):
        assert a.tobytes() == b.tobytes()
        hdr_a, hdr_c = a.view(np.uint32)[:16], c.view(np.uint32)[:16]
        assert hdr_a[14] == hdr_a[15] == 0 and hdr_c[14] & 1 and hdr_c[15] > 0
        assert len(c) == len(a) and np.array_equal(hdr_c[:14], hdr_a[:14]) and c[64:].tobytes() == a[64:].tobytes()
