"""Streams of the ObserveImage queue (vsf_observe_set_streams / vsf_observe_submit_stream): one context and one queue take
frames of several independent sequences, and frames of different streams leave for the GPU in the same batch.  The whole
correctness statement: each stream's results are, byte for byte, what a context of its own produces -- so the reference
throughout is a fresh one-stream context fed only that stream's frames through vsf_observe_stereo, and there is no tolerance
to choose.  Every result is compared whole, header words included."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

W, H, NF, LIFE, N = 320, 240, 700, 3, 8
F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
F_SHIFT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 1.5]], np.float32)  # a constant on every residual: another threshold chain
# the non-symmetric F of tests/test_gpu_frontend_dev.py (Eigen's summation order matters on it)
F_DENSE = np.array([[2.31e-08, -1.17e-05, 3.45e-03], [1.22e-05, 9.8e-08, -0.11], [-4.1e-03, 0.108, 1.0]], np.float32)
BPS = [float(np.float32(0.3)), float(np.float32(0.6)), float(np.float32(0.3))]
ROUND_ROBIN = [s for _ in range(N) for s in range(3)]
# runs of one stream, and stream 2 starts late
IRREGULAR = [0, 0, 0, 1, 0, 1, 1, 1, 0, 2, 2, 1, 2, 2, 2, 0, 1, 2, 0, 1, 2, 2, 0, 1]
assert all(IRREGULAR.count(s) == N for s in range(3))


def _calibs():
    from vision_slam_frontend_amd import frontend
    c0 = frontend.default_calibration().set("fundamental", F_RECT)
    c1 = frontend.default_calibration().set("fundamental", F_SHIFT)
    pr = c1.get("projection_right").copy()
    pr.flat[3] *= 1.25  # another baseline: other 3-D points
    c1.set("projection_right", pr)
    c1.set("distortion_left", [0.02, -0.01, 0.001, -0.002, 0.0])
    c2 = frontend.default_calibration().set("fundamental", F_DENSE)
    return [c0, c1, c2]


def _frames():
    from vision_slam_frontend_amd import synth
    out = []
    for s in range(3):
        sc = synth.Scene(W, H, n_objects=400, seed=synth.BASE_SEED + 17 * s)
        out.append([(sc.render(f, 0), sc.render(f, 1)) for f in range(N)])
    return out


def _params(batch):
    from vision_slam_frontend_amd import capi
    return capi.default_params(W, H, max_images=2 * batch, nfeatures=NF)


def _own_context(frames, calib, bp, life=LIFE):
    """THE reference: a fresh one-stream context fed `frames` through vsf_observe_stereo; the results' bytes."""
    from vision_slam_frontend_amd import capi
    out = []
    with capi.Context(_params(1)) as ctx:
        cap = int(capi.lib().vsf_observe_capacity(ctx._h, life))
        for left, right in frames:
            buf, n = np.zeros(cap, np.uint8), C.c_size_t()
            st = capi.lib().vsf_observe_stereo(ctx._h, left.ctypes.data, right.ctypes.data, W, H, left.strides[0], C.byref(calib),
                                               bp, life, buf.ctypes.data, cap, C.byref(n))
            assert st == capi.VSF_OK, st
            out.append(buf[:n.value].tobytes())
    return out


@pytest.fixture(scope="module")
def world():
    """Three image sequences, three calibrations, two best_percent values, and each stream's reference results (computed
    once, shared, never changed)."""
    frames, calibs = _frames(), _calibs()
    want = [_own_context(frames[s], calibs[s], BPS[s]) for s in range(3)]
    for s in range(3):  # the sequences are not trivial: features, a full window, temporal factors
        hdr = np.frombuffer(want[s][-1][:64], np.uint32)
        assert hdr[1] == LIFE + 1 and hdr[2] > 20, (s, hdr)
    assert len({w[0] for w in want}) == 3
    return frames, calibs, want


def _queue(depth, batch, thread=0, min_batch=0, n_streams=3):
    from vision_slam_frontend_amd import capi
    ctx = capi.Context(_params(batch))
    ctx.set_option(capi.OPT_OBSERVE_THREAD, thread)
    ctx.observe_configure(depth, min_batch, 0)
    ctx.observe_set_streams(n_streams)
    return ctx


def _drive(ctx, depth, order, frames, calibs, bps, life=LIFE, submit=None):
    """Submits frames in `order` (a list of streams; each stream's frames in sequence), at most `depth` uncollected; returns
    per stream the results' bytes in that stream's order."""
    got, tickets, nxt = [[] for _ in frames], [], [0] * len(frames)
    for s in order:
        if len(tickets) == depth:
            t, sc = tickets.pop(0)
            got[sc].append(ctx.observe_collect_bytes(t, life)[1].tobytes())
        left, right = frames[s][nxt[s]]
        nxt[s] += 1
        if submit:
            t = submit(ctx, s, left, right)
        else:
            t = ctx.observe_submit_stream(s, left, right, calibs[s], best_percent=bps[s], frame_life=life)
        assert t == (tickets[-1][0] + 1 if tickets else t)  # tickets are global and consecutive
        tickets.append((t, s))
    for t, sc in tickets:
        got[sc].append(ctx.observe_collect_bytes(t, life)[1].tobytes())
    return got


def _assert_streams_equal(got, want):
    for s, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (s, len(g), len(w))
        for k, (a, b) in enumerate(zip(g, w)):
            assert a == b, "stream %d frame %d differs from its own context's" % (s, k)


@pytest.mark.parametrize("thread", [0, 1])
@pytest.mark.parametrize("depth,batch", [(1, 1), (4, 4), (32, 32), (32, 8)])
@pytest.mark.parametrize("order", ["round_robin", "irregular"])
def test_interleaved_streams_equal_separate_contexts(world, order, depth, batch, thread):
    """Three streams -- different images, three calibrations (one with a non-symmetric F), two best_percent values -- through
    one queue, round-robin and in an irregular order, at four queue shapes, launched by the caller and by the launcher
    thread: every ticket's whole result equals the bytes of the stream's own context."""
    frames, calibs, want = world
    with _queue(depth, batch, thread) as ctx:
        got = _drive(ctx, depth, ROUND_ROBIN if order == "round_robin" else IRREGULAR, frames, calibs, BPS)
        stats = ctx.observe_stats()
    _assert_streams_equal(got, want)
    assert stats["frames"] == 3 * N and stats["streams"] == 3


def test_streams_really_share_batches(world):
    """Depth 32, 24 frames of three calibrations submitted before any collect (nothing leaves a busy-or-not queue that waits
    for 32 frames until the first collect sends everything): ONE batch of 24 that carried three streams."""
    frames, calibs, want = world
    with _queue(32, 32, min_batch=32) as ctx:
        got = _drive(ctx, 32, ROUND_ROBIN, frames, calibs, BPS)
        stats = ctx.observe_stats()
    assert stats["max_batch"] == 24 and stats["batches"] == 1 and stats["multi_stream_batches"] >= 1, stats
    _assert_streams_equal(got, want)


def test_nan_chain_is_isolated(world):
    """Stream 1 gets an all-zero frame in the middle of a shared batch: no stereo match, a NaN threshold for ITS next frame
    (quirk Q3), which keeps nothing, and the frame after recovers -- as in its own context; the other streams' bytes are
    those of the undisturbed run."""
    frames, calibs, want = world
    mine = list(frames[1])
    mine[3] = (np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8))
    want1 = _own_context(mine, calibs[1], BPS[1])
    nfeat = [int(np.frombuffer(r[:64], np.uint32)[2]) for r in want1]
    thr = [float(np.frombuffer(r[:64], np.float32)[9]) for r in want1]
    assert nfeat[3] == 0 and nfeat[4] == 0 and nfeat[5] > 20 and np.isnan(thr[4]) and np.isfinite(thr[5]), (nfeat, thr)
    with _queue(32, 32, min_batch=32) as ctx:
        got = _drive(ctx, 32, ROUND_ROBIN, [frames[0], mine, frames[2]], calibs, BPS)
        assert ctx.observe_stats()["max_batch"] == 24
    _assert_streams_equal(got, [want[0], want1, want[2]])


def test_windows_are_isolated(world):
    """frame_life 2, streams of 8, 5 and 2 frames: a result has min(frames of ITS stream so far, 2) + 1 pair lists, and the
    factor bytes are its own context's."""
    frames, calibs, _ = world
    lens = [8, 5, 2]
    seqs = [frames[s][:lens[s]] for s in range(3)]
    want = [_own_context(seqs[s], calibs[s], BPS[s], life=2) for s in range(3)]
    order = [0, 1, 2, 0, 1, 0, 2, 0, 1, 0, 1, 0, 1, 0, 0]
    assert [order.count(s) for s in range(3)] == lens
    for depth, batch in ((8, 8), (3, 2)):
        with _queue(depth, batch) as ctx:
            got = _drive(ctx, depth, order, seqs, calibs, BPS, life=2)
        for s in range(3):
            for k, r in enumerate(got[s]):
                assert int(np.frombuffer(r[:64], np.uint32)[1]) == min(k, 2) + 1, (s, k)
        _assert_streams_equal(got, want)


def test_reset_stream(world):
    """vsf_observe_reset_stream: refused while a frame of that stream is uncollected; afterwards the stream's next frame is the
    first frame of a fresh context, while the other streams -- with frames in flight across the reset -- continue unchanged."""
    from vision_slam_frontend_amd import capi
    frames, calibs, want = world
    fresh1 = _own_context(frames[1][4:], calibs[1], BPS[1])
    with _queue(16, 8) as ctx:
        sub = lambda s, k: ctx.observe_submit_stream(s, *frames[s][k], calibs[s], best_percent=BPS[s], frame_life=LIFE)  # noqa: E731
        col = lambda t: ctx.observe_collect_bytes(t, LIFE)[1].tobytes()  # noqa: E731
        first = [(s, k, sub(s, k)) for k in range(4) for s in range(3) if not (s == 1 and k == 3)]
        t13 = sub(1, 3)
        with pytest.raises(capi.VsfError):
            ctx.observe_reset_stream(1)  # frames of stream 1 wait or fly
        for s, k, t in first:
            assert col(t) == want[s][k], (s, k)
        with pytest.raises(capi.VsfError):
            ctx.observe_reset_stream(1)  # its frame 3 is still uncollected
        assert col(t13) == want[1][3]
        with pytest.raises(capi.VsfError):
            ctx.observe_reset_stream(3)
        t04, t24 = sub(0, 4), sub(2, 4)  # the others have frames in the queue across the reset
        ctx.observe_reset_stream(1)
        rest = [(s, k, sub(s, k)) for k in range(4, N) for s in range(3) if not (s != 1 and k == 4)]
        assert col(t04) == want[0][4] and col(t24) == want[2][4]
        for s, k, t in rest:
            assert col(t) == (fresh1[k - 4] if s == 1 else want[s][k]), (s, k)
    assert fresh1[1] != want[1][5]  # (the reset is visible: a shorter window, another threshold)


def test_compressed_and_raw_across_streams(world):
    """Stream 0 is fed JPEG files, stream 1 PNG files, stream 2 raw frames, all in shared batches: results equal
    vsf_observe_submit on the decoded images, per stream."""
    import test_gpu_observe_compressed as oc
    frames, calibs, want = world
    files = [[(oc._encode(l, fmt), oc._encode(r, fmt)) for l, r in frames[s]] for s, fmt in ((0, "jpeg"), (1, "png"))]
    decoded = [[(oc._decode(l), oc._decode(r)) for l, r in fs] for fs in files]
    want = [_own_context(decoded[0], calibs[0], BPS[0]), _own_context(decoded[1], calibs[1], BPS[1]), want[2]]
    assert want[1] == world[2][1]  # (PNG is lossless: stream 1's reference is the raw one)

    def submit(ctx, s, left, right):
        if s == 2:
            return ctx.observe_submit_stream(s, left, right, calibs[s], best_percent=BPS[s], frame_life=LIFE)
        st, t = ctx.observe_submit_compressed_stream(s, left, right, calibs[s], best_percent=BPS[s], frame_life=LIFE)
        return t

    for depth, batch in ((32, 32), (4, 4)):
        with _queue(depth, batch, min_batch=batch) as ctx:
            got = _drive(ctx, depth, IRREGULAR, [files[0], files[1], frames[2]], calibs, BPS, submit=submit)
            stats = ctx.observe_stats()
        assert stats["compressed"] == 2 * N and stats["multi_stream_batches"] >= 1
        _assert_streams_equal(got, want)


def test_refusals_leave_the_queue_untouched(world):
    """A stream out of range issues no ticket; vsf_observe_set_streams with frames in flight, with 0 and with 65 streams is
    refused; debug images and several streams refuse each other in both orders; after every refused call the next valid
    frame's result is what it would have been."""
    from vision_slam_frontend_amd import capi
    frames, calibs, want = world
    INV, UNS = capi.VSF_ERR_INVALID_ARG, capi.VSF_ERR_UNSUPPORTED
    L = capi.lib()
    nxt = [0, 0, 0]
    with _queue(8, 8) as ctx:
        def valid(s):
            k = nxt[s]
            nxt[s] += 1
            t = ctx.observe_submit_stream(s, *frames[s][k], calibs[s], best_percent=BPS[s], frame_life=LIFE)
            return s, k, t

        def check(skt):
            s, k, t = skt
            assert ctx.observe_collect_bytes(t, LIFE)[1].tobytes() == want[s][k], (s, k)

        a = valid(0)
        for bad in (3, -1, 64):
            assert ctx.observe_submit_stream(bad, *frames[0][1], calibs[0], best_percent=BPS[0], frame_life=LIFE,
                                             allow_status=(INV,)) == (INV, -1)
        assert ctx.observe_submit_compressed_stream(3, b"\xff\xd8", b"\xff\xd8", calibs[0], allow_status=(INV,)) == (INV, -1)
        b = valid(1)
        assert b[2] == a[2] + 1  # the refused submits took no ticket
        assert ctx.observe_set_streams(2, allow_status=(INV,)) == INV  # frames in flight
        c = valid(2)
        for skt in (a, b, c):
            check(skt)
        for n in (0, 65, -3):
            assert ctx.observe_set_streams(n, allow_status=(INV,)) == INV
        # debug images are single-stream: refused with three streams, in all three forms
        assert L.vsf_observe_set_debug_images(ctx._h, 1) == UNS
        assert L.vsf_observe_set_debug_jpeg(ctx._h, 90) == UNS
        assert L.vsf_observe_set_debug_png(ctx._h, 1) == UNS
        assert ctx.observe_set_streams(3) == capi.VSF_OK  # (the value it has: nothing is rebuilt)
        for skt in (valid(0), valid(1), valid(2), valid(1)):  # windows and thresholds are still there
            check(skt)
        assert ctx.observe_stats()["streams"] == 3
    # the other order: debug images on, then more than one stream
    with capi.Context(_params(4)) as ctx:
        assert L.vsf_observe_set_debug_images(ctx._h, 1) == capi.VSF_OK
        assert ctx.observe_set_streams(2, allow_status=(UNS,)) == UNS
        assert ctx.observe_set_streams(1) == capi.VSF_OK
        assert L.vsf_observe_set_debug_png(ctx._h, 1) == capi.VSF_OK
        assert ctx.observe_set_streams(3, allow_status=(UNS,)) == UNS
        assert L.vsf_observe_set_debug_png(ctx._h, 0) == capi.VSF_OK and L.vsf_observe_set_debug_images(ctx._h, 0) == capi.VSF_OK
        assert ctx.observe_set_streams(3) == capi.VSF_OK
        t = ctx.observe_submit_stream(2, *frames[2][0], calibs[2], best_percent=BPS[2], frame_life=LIFE)
        assert ctx.observe_collect_bytes(t, LIFE)[1].tobytes() == want[2][0]


def test_one_stream_is_the_queue_as_it_was(world):
    """vsf_observe_set_streams(1) and the _stream calls with stream 0 give the bytes of the existing calls, at a depth where
    batches form; and a queue of three streams that only ever sees stream 0 does too."""
    frames, calibs, want = world
    for n_streams in (1, 3):
        with _queue(8, 4, n_streams=n_streams) as ctx:
            got = _drive(ctx, 8, [0] * N, [frames[0]], [calibs[0]], [BPS[0]])
            assert ctx.observe_stats()["multi_stream_batches"] == 0
        with _queue(8, 4, n_streams=1) as ctx:
            old = _drive(ctx, 8, [0] * N, [frames[0]], [calibs[0]], [BPS[0]],
                         submit=lambda c, s, l, r: c.observe_submit(l, r, calibs[0], best_percent=BPS[0], frame_life=LIFE))
        assert got[0] == old[0] == want[0]
