"""Frames that already live in device memory entering the ObserveImage queue (vsf_observe_submit_dev).  The reference in every
case is the EXISTING queue fed the same pixels as raw host frames (vsf_observe_submit); collected results are compared with
==, whole and header words included: the pixels are identical, so the results must be, and there is no tolerance to choose.
Two contexts: 320 x 240, and 326 x 246 whose width is no multiple of 4 or 16 (the last 16-byte piece of a row is partial and
the rows' addresses take every alignment)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

SIZES = [(320, 240), (326, 246)]
NF, LIFE, N = 700, 3, 11
F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
F_SHIFT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 1.5]], np.float32)
F_DENSE = np.array([[2.31e-08, -1.17e-05, 3.45e-03], [1.22e-05, 9.8e-08, -0.11], [-4.1e-03, 0.108, 1.0]], np.float32)
BP = float(np.float32(0.3))
OFFSETS, POISON = (0, 1, 3, 7, 13), (0xA5, 0x3C)


def _pitches(w):
    return (w, w + 1, w + 37, 4096)


def _calib(F=F_RECT):
    from vision_slam_frontend_amd import frontend
    return frontend.default_calibration().set("fundamental", F)


def _scene(w, h, n=N, seed=0):
    from vision_slam_frontend_amd import synth
    sc = synth.Scene(w, h, n_objects=400, seed=synth.BASE_SEED + seed)
    return [(sc.render(f, 0), sc.render(f, 1)) for f in range(n)]


def _context(w, h, depth, batch=None, streams=1, min_batch=0):
    from vision_slam_frontend_amd import capi
    ctx = capi.Context(capi.default_params(w, h, max_images=2 * min(batch or depth, 16), nfeatures=NF))
    ctx.observe_configure(depth, min_batch, 0)
    if streams > 1:
        ctx.observe_set_streams(streams)
    return ctx


def _raw_results(w, h, frames, calib=None, bp=BP):
    """THE reference: the existing queue fed `frames` as raw host images, one at a time; the results' bytes."""
    calib = calib or _calib()
    with _context(w, h, 1) as ctx:
        out = []
        for left, right in frames:
            t = ctx.observe_submit(left, right, calib, best_percent=bp, frame_life=LIFE)
            out.append(ctx.observe_collect_bytes(t, LIFE)[1].tobytes())
    return out


@pytest.fixture(scope="module")
def world():
    """Per context size: the frames and their raw-queue results (computed once, shared, never changed)."""
    out = {}
    for w, h in SIZES:
        frames = _scene(w, h)
        want = _raw_results(w, h, frames)
        hdr = np.frombuffer(want[-1][:64], np.uint32)
        assert hdr[1] == LIFE + 1 and hdr[2] > 20, hdr  # not trivial: features, a full window, temporal factors
        out[(w, h)] = (frames, want)
    return out


def _view(img, offset=0, pitch=None, poison=0xA5, tail=64):
    """`img` in device memory as a strided view: `offset` bytes into its storage, rows `pitch` apart, every byte around and
    between the rows poisoned; tail: bytes of storage behind the last pixel (0: it IS the storage's last byte)."""
    import torch
    h, w = img.shape
    pitch = pitch or w
    host = np.full(offset + (h - 1) * pitch + w + tail, poison, np.uint8)
    rows = np.lib.stride_tricks.as_strided(host[offset:], (h, w), (pitch, 1))
    rows[:] = img
    dev = torch.from_numpy(host).to("cuda:0")
    return torch.as_strided(dev, (h, w), (pitch, 1), offset)


def _drive(ctx, depth, frames, submit):
    """submit(i, left, right) -> tickets of frame i; at most `depth` uncollected; the results' bytes in order."""
    got, tickets = [], []
    for i, (left, right) in enumerate(frames):
        if len(tickets) == depth:
            got.append(ctx.observe_collect_bytes(tickets.pop(0), LIFE)[1].tobytes())
        new = submit(i, left, right)
        assert new == [(tickets[-1] + 1 if tickets else new[0])]
        tickets += new
    got += [ctx.observe_collect_bytes(t, LIFE)[1].tobytes() for t in tickets]
    return got


def _assert_equal(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "frame %d differs from the raw queue's" % i


# ---- 1. device = raw ----
@pytest.mark.parametrize("size", SIZES, ids=["320x240", "326x246"])
@pytest.mark.parametrize("depth", [1, 4, 32])
def test_device_frames_equal_raw_frames(world, size, depth):
    """11 frames (a window of 3: more frames than the window; at depth 4 the ring wraps twice) as contiguous device tensors
    at depths 1 / 4 / 32 -- batches of one, of up to four, and whatever the policy releases of eleven."""
    frames, want = world[size]
    calib = _calib()
    with _context(*size, depth) as ctx:
        got = _drive(ctx, depth, frames, lambda i, l, r: ctx.observe_submit_dev([(_view(l), _view(r))], calib, best_percent=BP,
                                                                                frame_life=LIFE))
        s = ctx.observe_stats()
    _assert_equal(got, want)
    assert s["device_frames"] == N and s["frames"] == N and s["compressed"] == 0
    assert s["max_batch"] == (1 if depth == 1 else s["max_batch"]) and s["max_batch"] <= min(depth, 16)


# ---- 2. addressing ----
@pytest.mark.parametrize("size", SIZES, ids=["320x240", "326x246"])
def test_any_base_address_and_pitch(world, size):
    """Base offsets 0 / 1 / 3 / 7 / 13 and pitches w, w + 1, w + 37, 4096, left and right differing in both, every byte
    around the pixels poisoned -- with two patterns in two runs: a byte from outside an image would change a result in at
    least one of them.  One frame's left image ends on the last byte of its tensor's storage."""
    frames, want = world[size]
    calib, pitches = _calib(), _pitches(size[0])
    for poison in POISON:
        def submit(i, l, r):
            lv = _view(l, OFFSETS[i % 5], pitches[i % 4], poison, tail=0 if i in (3, 8) else 64)
            rv = _view(r, OFFSETS[(i + 2) % 5], pitches[(i + 1) % 4], poison, tail=0 if i == 9 else 64)
            if i in (3, 8):
                st = lv.untyped_storage()
                assert lv.data_ptr() + (size[1] - 1) * lv.stride(0) + size[0] == st.data_ptr() + st.nbytes()
            return ctx.observe_submit_dev([(lv, rv)], calib, best_percent=BP, frame_life=LIFE)
        with _context(*size, 4) as ctx:
            got = _drive(ctx, 4, frames, submit)
        _assert_equal(got, want)


# ---- 3. stream order ----
@pytest.mark.parametrize("depth", [4, 32])
def test_stream_ordered_on_the_producers_stream(world, depth):
    """ONE pair of device buffers for every frame: each frame is copied in with a non-blocking copy on a side stream, submitted
    with that stream, and the buffers are overwritten on the same stream immediately afterwards; the host never synchronises
    before the collects."""
    import torch
    size = SIZES[1]
    frames, want = world[size]
    calib = _calib()
    side = torch.cuda.Stream()
    pinned = [(torch.from_numpy(l).pin_memory(), torch.from_numpy(r).pin_memory()) for l, r in frames]
    buf_l = torch.empty((size[1], size[0]), dtype=torch.uint8, device="cuda:0")
    buf_r = torch.empty_like(buf_l)
    torch.cuda.synchronize()

    def submit(i, l, r):
        with torch.cuda.stream(side):
            buf_l.copy_(pinned[i][0], non_blocking=True)
            buf_r.copy_(pinned[i][1], non_blocking=True)
            t = ctx.observe_submit_dev([(buf_l, buf_r)], calib, producer_stream=side.cuda_stream, best_percent=BP, frame_life=LIFE)
            buf_l.fill_(0x5A)
            buf_r.fill_(0xC3)
        return t
    with _context(*size, depth) as ctx:
        got = _drive(ctx, depth, frames, submit)
    _assert_equal(got, want)


def test_images_still_being_produced_on_the_stream(world):
    """The images are the result of tensor arithmetic queued on a side stream (255 - x of an inverted upload); submitted
    without waiting, with stream=None resolved from torch's current stream."""
    import torch
    size = SIZES[0]
    frames, want = world[size]
    calib = _calib()
    side = torch.cuda.Stream()
    inverted = [(torch.from_numpy(255 - l).to("cuda:0"), torch.from_numpy(255 - r).to("cuda:0")) for l, r in frames]
    torch.cuda.synchronize()

    def submit(i, l, r):
        with torch.cuda.stream(side):
            lt, rt = 255 - inverted[i][0], 255 - inverted[i][1]
            return ctx.observe_submit_dev([(lt, rt)], calib, best_percent=BP, frame_life=LIFE)  # (current stream: side)
    with _context(*size, 32) as ctx:
        got = _drive(ctx, 32, frames, submit)
    _assert_equal(got, want)


# ---- 4. several frames per call ----
def test_several_frames_per_call(world):
    """n = 5 issues consecutive tickets and equals five calls of one (a table in pinned memory: 10 images); n = 3 rides in
    the kernel arguments.  n = free slots + 1 is refused with INVALID_ARG and the queue is as before: a following raw submit
    gets the next ticket and the right result."""
    from vision_slam_frontend_amd import capi
    size = SIZES[1]
    frames, want = world[size]
    calib = _calib()
    views = [(_view(l, 3, size[0] + 1), _view(r, 0, 4096)) for l, r in frames]
    with _context(*size, 8) as ctx:
        t = ctx.observe_submit_dev(views[0:5], calib, best_percent=BP, frame_life=LIFE)
        assert t == [0, 1, 2, 3, 4]
        t += ctx.observe_submit_dev(views[5:8], calib, best_percent=BP, frame_life=LIFE)
        assert t == list(range(8))
        st, none = ctx.observe_submit_dev(views[8:9], calib, best_percent=BP, frame_life=LIFE, allow_status=(capi.VSF_ERR_INVALID_ARG,))
        assert st == capi.VSF_ERR_INVALID_ARG and none == [-1]  # the queue is full
        got = [ctx.observe_collect_bytes(k, LIFE)[1].tobytes() for k in t[:6]]
        # six slots are free: seven frames are one too many -- nothing of the call is taken, nothing is launched
        timers = ("copy_ns", "launch_ns", "wait_ns")
        before = {k: v for k, v in ctx.observe_stats().items() if k not in timers}
        st, none = ctx.observe_submit_dev([views[8]] * 7, calib, best_percent=BP, frame_life=LIFE, allow_status=(capi.VSF_ERR_INVALID_ARG,))
        assert st == capi.VSF_ERR_INVALID_ARG and none == [-1] * 7
        assert {k: v for k, v in ctx.observe_stats().items() if k not in timers} == before
        got += [ctx.observe_collect_bytes(k, LIFE)[1].tobytes() for k in t[6:]]
        t8 = ctx.observe_submit(*frames[8], calib, best_percent=BP, frame_life=LIFE)  # raw, behind the refusal
        assert t8 == 8
        t9 = ctx.observe_submit_dev(views[9:11], calib, best_percent=BP, frame_life=LIFE)
        assert t9 == [9, 10]
        got += [ctx.observe_collect_bytes(k, LIFE)[1].tobytes() for k in [t8] + t9]
        assert ctx.observe_stats()["device_frames"] == 10
    _assert_equal(got, want)


# ---- 5. ring wrap and mixing ----
def test_ring_wrap_at_depth_4(world):
    """Depth 4, 11 device frames, three per call where there is room: calls and batches that wrap the ring."""
    size = SIZES[0]
    frames, want = world[size]
    calib = _calib()
    views = [(_view(l, 1, size[0] + 37), _view(r, 13, size[0])) for l, r in frames]
    got, tickets, i = [], [], 0
    with _context(*size, 4, min_batch=4) as ctx:
        while i < N:
            n = min(3, N - i, 4 - len(tickets))
            tickets += ctx.observe_submit_dev(views[i:i + n], calib, best_percent=BP, frame_life=LIFE)
            i += n
            for _ in range(2 if i < N else len(tickets)):
                got.append(ctx.observe_collect_bytes(tickets.pop(0), LIFE)[1].tobytes())
        s = ctx.observe_stats()
    _assert_equal(got, want)
    assert s["device_frames"] == N and s["device_ring_bytes"] == 4 * 2 * 320 * 240


def _files_and_pixels(size, frames):
    """Per frame a JPEG pair and a PNG pair (this project's encoders) and the pixels this project's decoders read from them."""
    import torch
    from vision_slam_frontend_amd import capi
    w, h = size
    with capi.Context(capi.default_params(w, h, max_images=2, nfeatures=100)) as c:
        flat = [im for pair in frames for im in pair]
        files = {"jpeg": c.jpeg_encode(flat, quality=90), "png": c.png_encode(flat)}
        pixels = {}
        for k, fs in files.items():
            pitch = (w + 63) & ~63  # (the decoders want 4-byte aligned rows)
            d = torch.zeros((len(fs), h, pitch), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            c.imdecode_gray_batch(fs, w, h, d.data_ptr(), pitch * h, pitch)
            assert c.sync() == capi.VSF_OK
            pixels[k] = np.ascontiguousarray(d.cpu().numpy()[:, :, :w])
    return files, pixels


def test_raw_jpeg_png_and_device_frames_in_one_queue(world):
    """Depth 32: raw, JPEG, PNG and device frames interleaved in one queue (and one batch) equal the all-raw run on the decoded
    pixels; observe_stats()[17] counts exactly the device frames."""
    size = SIZES[1]
    frames, _ = world[size]
    calib = _calib()
    files, pixels = _files_and_pixels(size, frames)
    kinds = ["raw", "jpeg", "png", "dev", "dev", "png", "raw", "dev", "jpeg", "dev", "raw"]
    pix = [frames[i] if k in ("raw", "dev") else (pixels[k][2 * i], pixels[k][2 * i + 1]) for i, k in enumerate(kinds)]
    want = _raw_results(*size, pix)
    tickets = []
    with _context(*size, 32) as ctx:
        for i, k in enumerate(kinds):
            if k == "raw":
                tickets.append(ctx.observe_submit(*frames[i], calib, best_percent=BP, frame_life=LIFE))
            elif k == "dev":
                tickets += ctx.observe_submit_dev([(_view(frames[i][0], 7, size[0] + 1), _view(frames[i][1]))], calib,
                                                  best_percent=BP, frame_life=LIFE)
            else:
                st, t = ctx.observe_submit_compressed(files[k][2 * i], files[k][2 * i + 1], calib, best_percent=BP, frame_life=LIFE)
                tickets.append(t)
        assert tickets == list(range(N))
        got = [ctx.observe_collect_bytes(t, LIFE)[1].tobytes() for t in tickets]
        v = np.zeros(20, np.int64)
        assert capi_lib().vsf_observe_stats(ctx._h, v.ctypes.data, 20) == 0
        s = ctx.observe_stats()
    _assert_equal(got, want)
    assert v[17] == kinds.count("dev") == s["device_frames"] and s["compressed"] == 4 and s["max_batch"] > 4
    assert v[19] == s["device_ring_bytes"] > 0 and v[18] == s["device_commands"] >= kinds.count("dev")


def capi_lib():
    from vision_slam_frontend_amd import capi
    return capi.lib()


# ---- 6. Bayer ----
def test_bayer_mosaics_and_the_cut_behind_them(world):
    """Device mosaics with VSF_PIX_BAYER_RGGB8 equal a raw submit of the CPU demosaic of the same mosaics; a mono frame behind
    a Bayer frame starts a new batch (everything waits together at depth 8: only the submit-side rule separates them)."""
    from oracle import binding as ob
    from vision_slam_frontend_amd import capi
    size = SIZES[1]
    frames, _ = world[size]
    calib = _calib()
    kinds = ["bay", "bay", "bay", "mono", "mono", "bay", "mono", "mono"]
    pix = [(ob.bayer_bg_to_gray(l), ob.bayer_bg_to_gray(r)) if k == "bay" else (l, r) for k, (l, r) in zip(kinds, frames)]
    want = _raw_results(*size, pix)
    with _context(*size, 8, min_batch=8) as ctx:
        tickets = []
        for i, k in enumerate(kinds):
            tickets += ctx.observe_submit_dev([(_view(frames[i][0], 1, size[0] + 1), _view(frames[i][1], 0, 4096))], calib,
                                              pixfmt=capi.PIX_BAYER_RGGB8 if k == "bay" else capi.PIX_MONO8, best_percent=BP,
                                              frame_life=LIFE)
        got = [ctx.observe_collect_bytes(t, LIFE)[1].tobytes() for t in tickets]
        s = ctx.observe_stats()
    _assert_equal(got, want)
    assert got[0] != _raw_results(*size, frames[:1])[0]  # (the flag matters)
    assert s["batches"] == 4 and s["max_batch"] == 3, s  # bay bay bay | mono mono | bay | mono mono


# ---- 7. streams ----
def test_three_streams_round_robin(world):
    """Three streams with distinct calibrations and best_percent, device frames round-robin through one queue: each stream
    equals a raw queue of its own (the pattern of tests/test_gpu_observe_streams.py)."""
    size = SIZES[0]
    calibs = [_calib(F_RECT), _calib(F_SHIFT), _calib(F_DENSE)]
    bps = [float(np.float32(0.3)), float(np.float32(0.6)), float(np.float32(0.3))]
    seqs = [_scene(*size, n=6, seed=17 * s) for s in range(3)]
    want = [_raw_results(*size, seqs[s], calibs[s], bps[s]) for s in range(3)]
    got, tickets = [[] for _ in range(3)], []
    with _context(*size, 8, streams=3) as ctx:
        for k in range(6):
            for s in range(3):
                if len(tickets) == 8:
                    t, sc = tickets.pop(0)
                    got[sc].append(ctx.observe_collect_bytes(t, LIFE)[1].tobytes())
                l, r = seqs[s][k]
                t = ctx.observe_submit_dev([(_view(l, s, size[0] + s), _view(r))], calibs[s], stream=s, best_percent=bps[s],
                                           frame_life=LIFE)
                tickets.append((t[0], s))
        for t, sc in tickets:
            got[sc].append(ctx.observe_collect_bytes(t, LIFE)[1].tobytes())
        assert ctx.observe_stats()["multi_stream_batches"] > 0
    for s in range(3):
        _assert_equal(got[s], want[s])


# ---- 8. debug images ----
def _debug_run(size, frames, device, jpeg):
    from vision_slam_frontend_amd import capi
    L, calib, (w, h) = capi.lib(), _calib(), size
    C.CDLL("libc.so.6").srand(7)
    out = []
    with capi.Context(capi.default_params(w, h, max_images=4, nfeatures=NF)) as ctx:
        ctx.observe_configure(2, 0, 0)
        assert L.vsf_observe_set_debug_images(ctx._h, 1) == capi.VSF_OK
        if jpeg:
            assert L.vsf_observe_set_debug_jpeg(ctx._h, 90) == capi.VSF_OK
        if device:
            tickets = ctx.observe_submit_dev([(_view(l, 3, w + 37), _view(r, 1, w + 1)) for l, r in frames], calib, best_percent=BP,
                                             frame_life=LIFE)
        else:
            tickets = [ctx.observe_submit(l, r, calib, best_percent=BP, frame_life=LIFE) for l, r in frames]
        for t in tickets:
            res = ctx.observe_collect_bytes(t, LIFE)[1].tobytes()
            s_, m_, sn, mn = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
            if jpeg:
                assert L.vsf_observe_debug_jpeg_view(ctx._h, t, C.byref(s_), C.byref(sn), C.byref(m_), C.byref(mn)) == capi.VSF_OK
            else:
                assert L.vsf_observe_debug_view(ctx._h, t, C.byref(s_), C.byref(m_)) == capi.VSF_OK
                sn, mn = C.c_size_t(6 * w * h), C.c_size_t(3 * w * h)
            out.append((res, C.string_at(s_.value, sn.value) if s_.value else None, C.string_at(m_.value, mn.value) if m_.value else None))
    return out


@pytest.mark.parametrize("jpeg", [False, True], ids=["canvases", "jpeg_files"])
def test_debug_images_of_device_frames(world, jpeg):
    """With the debug images on, two device frames give the same results, the same canvases and the same JPEG files as the
    same frames submitted raw (they are drawn from the batch's image buffer either way)."""
    size = SIZES[1]
    frames = world[size][0][:2]
    got, want = _debug_run(size, frames, True, jpeg), _debug_run(size, frames, False, jpeg)
    assert got == want
    assert got[0][1] is not None and got[1][2] is not None  # a stereo image, and a match image from the second frame on


# ---- 9. refusals ----
def test_refusals_leave_no_ticket_and_no_ring(world):
    from vision_slam_frontend_amd import capi
    L = capi.lib()
    size = SIZES[0]
    w, h = size
    frames, want = world[size]
    calib, INV = _calib(), capi.VSF_ERR_INVALID_ARG
    files, _ = _files_and_pixels(size, frames[:1])
    views = [(_view(l), _view(r)) for l, r in frames[:4]]
    lp, rp = views[0][0].data_ptr(), views[0][1].data_ptr()

    def raw_call(ctx, frames_arr, n, pixfmt=0, stream=0, cal=calib, life=LIFE, tickets=True, ctx_null=False):
        t = (C.c_int64 * 8)(*([77] * 8))
        st = L.vsf_observe_submit_dev(None if ctx_null else ctx._h, stream, frames_arr, n, pixfmt, None,
                                      C.byref(cal) if cal is not None else None, BP, life, t if tickets else None)
        return st, list(t)[:max(n, 1)]

    def arr(*fr):
        a = (capi.VsfDevFrame * len(fr))()
        for i, f in enumerate(fr):
            a[i] = capi.VsfDevFrame(f[0], f[1], f[2], f[3])
        return a
    good = (lp, rp, w, w)
    with _context(*size, 4, streams=2) as ctx:
        # a queue that has seen only raw and compressed frames: no device counters, no ring
        t0 = ctx.observe_submit(*frames[0], calib, best_percent=BP, frame_life=LIFE)
        st, t1 = ctx.observe_submit_compressed(files["jpeg"][0], files["png"][1], calib, best_percent=BP, frame_life=LIFE)
        for t in (t0, t1):
            ctx.observe_collect_bytes(t, LIFE)
        s = ctx.observe_stats()
        assert (s["device_frames"], s["device_commands"], s["device_ring_bytes"]) == (0, 0, 0) and s["frames"] == 2
        ctx.observe_reset()
        refused = [
            raw_call(ctx, arr(good), 1, ctx_null=True), raw_call(ctx, None, 1), raw_call(ctx, arr(good), 1, cal=None),
            raw_call(ctx, arr(good), 1, tickets=False),
            raw_call(ctx, arr((0, rp, w, w)), 1), raw_call(ctx, arr(good, (lp, 0, w, w)), 2),       # a null image
            raw_call(ctx, arr(good), 0), raw_call(ctx, arr(good), -1),                                # n < 1
            raw_call(ctx, arr(good, good, good, good, good), 5),                                      # n > free slots (4)
            raw_call(ctx, arr((lp, rp, w - 1, w)), 1), raw_call(ctx, arr(good, (lp, rp, w, w - 1)), 2),  # pitch < width
            raw_call(ctx, arr(good), 1, stream=2), raw_call(ctx, arr(good), 1, stream=-1),            # stream outside [0, 2)
            raw_call(ctx, arr(good), 1, pixfmt=2), raw_call(ctx, arr(good), 1, pixfmt=-1),            # unknown pixfmt
        ]
        bad_rows = capi.VsfCalibration.from_buffer_copy(bytes(calib))
        bad_rows.triangulate_rows = 5
        refused.append(raw_call(ctx, arr(good), 1, cal=bad_rows))
        for k, (st, t) in enumerate(refused):
            assert st == INV, (k, st)
            assert all(x in (-1, 77) for x in t), (k, t)  # no ticket (77: the call never reached the array)
        s = ctx.observe_stats()
        assert (s["frames"], s["device_frames"], s["device_commands"], s["device_ring_bytes"]) == (0, 0, 0, 0)
        assert ctx.observe_device_ring_bytes(4) == 4 * 2 * w * h and ctx.observe_device_ring_bytes(0) == 4 * 2 * w * h
        assert ctx.observe_device_ring_bytes(1025) == 0 and ctx.observe_device_ring_bytes(256) == 64 * 4 * 2 * w * h
        # the first device frame builds the ring; tickets start at 0: nothing above took one
        t = ctx.observe_submit_dev(views[:2], calib, best_percent=BP, frame_life=LIFE)
        assert t == [0, 1] and ctx.observe_stats()["device_ring_bytes"] == ctx.observe_device_ring_bytes(4)
        # another frame_life while frames wait
        st, none = ctx.observe_submit_dev(views[2:3], calib, best_percent=BP, frame_life=LIFE + 1, allow_status=(INV,))
        assert st == INV and none == [-1]
        t += ctx.observe_submit_dev(views[2:4], calib, best_percent=BP, frame_life=LIFE)
        st, none = ctx.observe_submit_dev(views[:1], calib, best_percent=BP, frame_life=LIFE, allow_status=(INV,))
        assert st == INV and none == [-1]  # full
        got = [ctx.observe_collect_bytes(k, LIFE)[1].tobytes() for k in t]
        assert t == [0, 1, 2, 3] and ctx.observe_stats()["device_frames"] == 4
    _assert_equal(got, want[:4])
    # max_keypoints >= 65536: UNSUPPORTED, as for raw frames
    with capi.Context(capi.default_params(w, h, max_images=2, nfeatures=65536)) as big:
        st, t = raw_call(big, arr(good), 1)
        assert st == capi.VSF_ERR_UNSUPPORTED and t == [-1]
    # a sticky queue status is handed back: the injected launch failure of the raw path's own test
    with _context(*size, 4, min_batch=4) as ctx:
        assert ctx.observe_submit_dev(views[:1], calib, best_percent=BP, frame_life=LIFE) == [0]  # (it waits for company)
        assert L.vsf_debug_inject_hip_error(ctx._h, 719) == capi.VSF_OK  # the host-side test hook: the next launch reports it
        st, _ = ctx.observe_collect_bytes(0, LIFE, allow_status=(capi.VSF_ERR_HIP,))
        assert st == capi.VSF_ERR_HIP  # the collect sent the frame; its launch took the noted error: the queue's status sticks
        st, none = ctx.observe_submit_dev(views[1:2], calib, best_percent=BP, frame_life=LIFE, allow_status=(capi.VSF_ERR_HIP,))
        assert st == capi.VSF_ERR_HIP and none == [-1]


# ---- 10. existing paths unchanged ----
def _old_paths_run(size, frames, files):
    calib = _calib()
    out = []
    for compressed in (False, True):
        with _context(*size, 4, min_batch=4) as ctx:
            res = []
            for i0 in range(0, N, 4):
                if compressed:
                    tickets = [ctx.observe_submit_compressed(files["jpeg" if i & 1 else "png"][2 * i], files["jpeg"][2 * i + 1], calib,
                                                             best_percent=BP, frame_life=LIFE)[1] for i in range(i0, min(i0 + 4, N))]
                else:
                    tickets = [ctx.observe_submit(l, r, calib, best_percent=BP, frame_life=LIFE) for l, r in frames[i0:i0 + 4]]
                res += [ctx.observe_collect_bytes(t, LIFE)[1].tobytes() for t in tickets]
            v = np.zeros(20, np.int64)
            assert capi_lib().vsf_observe_stats(ctx._h, v.ctypes.data, 20) == 0
            out.append((res, v))
    return out


def test_existing_paths_are_unchanged(world):
    """With no device frame submitted, a raw-only and a compressed-only run (11 frames at depth 4, min_batch 4, four at a
    time: two batches of four and a forced batch of three) issue the same `batches`, `ingest_commands` and `file_commands`
    as ever: positions 1-16 of vsf_observe_stats less the three host timers (8-10: nanoseconds, not counts) are compared
    with what the queue's policy gives for this schedule and with a second identical run; 17-19 stay 0.  This test passes
    without the feature too (positions 17-19 then read the zeros the caller put there)."""
    size = SIZES[0]
    frames, want = world[size]
    files, _ = _files_and_pixels(size, frames)
    a, b = _old_paths_run(size, frames, files), _old_paths_run(size, frames, files)
    counts = [1, 2, 3, 4, 5, 6, 7, 11, 12, 14, 15, 16]  # (13: bytes of the compressed path's buffers, compared below)
    for (ra, va), (rb, vb) in zip(a, b):
        assert ra == rb and [va[i] for i in counts] == [vb[i] for i in counts] and va[13] == vb[13]
        assert list(va[17:20]) == [0, 0, 0]
    _assert_equal(a[0][0], want)
    (_, raw), (_, cmp_) = a
    # batches, largest, solo, forced, slot waits, depth, bmax | compressed, ingest_commands | file_commands, streams, multi
    assert [raw[i] for i in counts] == [3, 4, 0, 1, 0, 4, 4, 0, 0, 0, 1, 0], list(raw)
    # a compressed batch: one copy command + one decode per run of a format + the ingest finish
    assert [cmp_[i] for i in counts[:7]] == [3, 4, 0, 1, 0, 4, 4] and cmp_[11] == N and cmp_[14] == 0, list(cmp_)
    assert raw[13] == 0 and cmp_[13] > 0
