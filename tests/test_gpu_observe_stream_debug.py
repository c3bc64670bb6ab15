"""Debug images for every stream of the ObserveImage queue (vsf_observe_set_debug_seeds): each stream draws its stereo lines'
colours from a generator of its own on the device, and keeps its own previous frame for the match image.  The yardstick is
the one of tests/test_gpu_observe_streams.py: each stream equals, byte for byte, a context of its own -- here a fresh
one-stream context with the OLD switch (vsf_observe_set_debug_images and the process's rand()) after srand(seed of that
stream).  Results (header words 14 / 15 included) and both canvases or files are compared whole; there is no tolerance."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import debug_files_run as dfr  # noqa: E402
import test_gpu_observe_streams as ts  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, LIFE, N = ts.W, ts.H, ts.LIFE, ts.N
assert (W, H) == (dfr.W, dfr.H)
SEEDS = [1, 7, 4242]
# stream 2 takes two frames, sits out sixteen -- at least two whole batches at 1 and at 4 frames per batch, one at 8 -- and
# comes back: its kept frame and its generator must have survived the batches it was not in
SIT_OUT = [2, 2] + [0, 1] * 8 + [2] * 6
assert all(SIT_OUT.count(s) == N for s in range(3))
ORDERS = {"round_robin": ts.ROUND_ROBIN, "irregular": ts.IRREGULAR, "sit_out": SIT_OUT}


def _libc():
    return C.CDLL("libc.so.6")


def _pics(ctx, form, ticket):
    from vision_slam_frontend_amd import capi
    st, s, m = dfr.files_view(ctx, form, ticket) if form else dfr.canvases_view(ctx, ticket)
    assert st == capi.VSF_OK
    return (s if form or s is None else s.tobytes(), m if form or m is None else m.tobytes())


def _switch(ctx, form):
    from vision_slam_frontend_amd import capi
    L = capi.lib()
    assert L.vsf_observe_set_debug_images(ctx._h, 1) == capi.VSF_OK
    if form == "jpeg":
        assert L.vsf_observe_set_debug_jpeg(ctx._h, 90) == capi.VSF_OK
    if form == "png":
        assert L.vsf_observe_set_debug_png(ctx._h, 1) == capi.VSF_OK


def _own_context(frames, calib, bp, seed, form=None):
    """THE reference: a fresh one-stream context, the old switch, srand(seed) once the context exists and before its first
    frame (tests/debug_files_run.py: seed()).  -> per frame (result bytes, stereo, match)"""
    from vision_slam_frontend_amd import capi
    out = []
    with capi.Context(ts._params(1)) as ctx:
        assert ctx.sync() == capi.VSF_OK
        _libc().srand(seed)
        _switch(ctx, form)
        for left, right in frames:
            t = ctx.observe_submit(left, right, calib, best_percent=bp, frame_life=LIFE)
            res = ctx.observe_collect_bytes(t, LIFE)[1].tobytes()
            out.append((res,) + _pics(ctx, form, t))
    return out


def _seeded_queue(depth, batch, thread=0, form=None, seeds=SEEDS, n_streams=3):
    ctx = ts._queue(depth, batch, thread, n_streams=n_streams)
    ctx.observe_set_debug_seeds(seeds)
    _switch(ctx, form)
    return ctx


def _drive(ctx, depth, order, frames, calibs, bps, form=None, debug=True):
    """ts._drive, and each collected frame's two images beside its result."""
    got, tickets, nxt = [[] for _ in frames], [], [0] * len(frames)

    def collect():
        t, sc = tickets.pop(0)
        res = ctx.observe_collect_bytes(t, LIFE)[1].tobytes()
        got[sc].append((res,) + (_pics(ctx, form, t) if debug else (None, None)))

    for s in order:
        if len(tickets) == depth:
            collect()
        left, right = frames[s][nxt[s]]
        nxt[s] += 1
        tickets.append((ctx.observe_submit_stream(s, left, right, calibs[s], best_percent=bps[s], frame_life=LIFE), s))
    while tickets:
        collect()
    return got


def _assert_equal(got, want, what=""):
    for s, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (s, len(g), len(w))
        for k, (a, b) in enumerate(zip(g, w)):
            for part, x, y in zip(("result", "stereo image", "match image"), a, b):
                assert (x is None) == (y is None), "%s stream %d frame %d: %s present / absent" % (what, s, k, part)
                assert x == y, "%s stream %d frame %d: %s differs from its own context's" % (what, s, k, part)


@pytest.fixture(scope="module")
def world():
    """The three sequences and calibrations of test_gpu_observe_streams.py; stream 1's frame 3 has an all-zero right image.
    Each stream's reference, computed once and never changed."""
    frames, calibs = ts._frames(), ts._calibs()
    frames[1][3] = (frames[1][3][0], np.zeros((H, W), np.uint8))
    want = [_own_context(frames[s], calibs[s], ts.BPS[s], SEEDS[s]) for s in range(3)]
    hdr = [[np.frombuffer(r[0][:64], np.uint32) for r in w] for w in want]
    # no stereo match: no stereo image, no colours -- and its NaN threshold leaves the next frame without one as well
    assert (hdr[1][3][14] & 1) == 0 and hdr[1][3][15] == 0 and want[1][3][1] is None
    assert (hdr[1][4][14] & 1) == 0 and hdr[1][4][15] == 0 and hdr[1][5][14] == 3 and hdr[1][5][15] > 5
    for s in range(3):  # colours are taken, both images exist, and the streams' images are not each other's
        assert hdr[s][-1][14] == 3 and hdr[s][-1][15] > 5 and want[s][0][2] is None and want[s][1][2] is not None
    assert len({w[-1][1] for w in want}) == 3
    return frames, calibs, want


@pytest.mark.parametrize("thread", [0, 1])
@pytest.mark.parametrize("depth,batch", [(1, 1), (4, 4), (32, 8)])
@pytest.mark.parametrize("order", list(ORDERS))
def test_each_stream_equals_its_own_context(world, order, depth, batch, thread):
    """Results, presence bits and both canvases per stream, for three orders (4 / 4 with 24 frames wraps the result ring and
    crosses batch boundaries inside every stream), launched by the caller and by the launcher thread."""
    frames, calibs, want = world
    with _seeded_queue(depth, batch, thread) as ctx:
        got = _drive(ctx, depth, ORDERS[order], frames, calibs, ts.BPS)
        stats = ctx.observe_stats()
    _assert_equal(got, want, order)
    assert stats["frames"] == 3 * N and stats["seeded_colour_frames"] == 3 * N
    assert 1 <= stats["colour_commands"] == stats["batches"]
    if depth == 1:
        assert stats["batches"] == 3 * N


@pytest.mark.parametrize("form", ["jpeg", "png"])
def test_file_forms(world, form):
    """JPEG files at quality 90 and PNG files: the encoders take the canvases just drawn, so the files are the own context's."""
    frames, calibs, _ = world
    want = [_own_context(frames[s], calibs[s], ts.BPS[s], SEEDS[s], form) for s in range(3)]
    assert want[0][-1][1][:2] == (b"\xff\xd8" if form == "jpeg" else b"\x89P")
    with _seeded_queue(4, 4, form=form) as ctx:
        got = _drive(ctx, 4, ts.IRREGULAR, frames, calibs, ts.BPS, form=form)
        assert ctx.observe_stats()["debug_jpeg_commands"] > 0
    _assert_equal(got, want, form)


def test_reset_stream(world):
    """After vsf_observe_reset_stream(1), stream 1 is a fresh context seeded again; streams 0 and 2 continue byte-equal."""
    frames, calibs, want = world
    fresh1 = _own_context(frames[1][4:], calibs[1], ts.BPS[1], SEEDS[1])
    with _seeded_queue(16, 8) as ctx:
        head = _drive(ctx, 16, [s for _ in range(4) for s in range(3)], frames, calibs, ts.BPS)
        _assert_equal(head, [w[:4] for w in want], "before the reset")
        ctx.observe_reset_stream(1)
        rest = [[f[4:] for f in frames][s] for s in range(3)]
        tail = _drive(ctx, 16, [s for _ in range(4) for s in range(3)], rest, calibs, ts.BPS)
    _assert_equal(tail, [want[0][4:], fresh1, want[2][4:]], "after the reset")
    assert fresh1[1][1] != want[1][5][1]  # (the reset is visible)


def test_one_stream_with_a_seed(world):
    """One stream with a seed: the old switch's bytes after srand(seed) -- and the process's rand() is not touched: srand(5)
    before the run and one rand() after it give the first value of srand(5)."""
    from vision_slam_frontend_amd import capi
    frames, calibs, want = world
    libc = _libc()
    with ts._queue(8, 4, n_streams=1) as ctx:
        assert ctx.sync() == capi.VSF_OK
        libc.srand(5)
        ctx.observe_set_debug_seeds([SEEDS[2]])
        _switch(ctx, None)
        got = _drive(ctx, 8, [0] * N, [frames[2]], [calibs[2]], [ts.BPS[2]])
        after = libc.rand()
    libc.srand(5)
    assert after == libc.rand()
    _assert_equal(got, [want[2]])


def test_seeds_without_debug_images_change_nothing(world):
    """Seeds installed, debug images off: the results of a queue that never saw the call; nothing of the path ran."""
    frames, calibs, _ = world
    runs = []
    for seeds in (None, SEEDS):
        with ts._queue(8, 8) as ctx:
            if seeds:
                ctx.observe_set_debug_seeds(seeds)
            runs.append(_drive(ctx, 8, ts.IRREGULAR, frames, calibs, ts.BPS, debug=False))
            stats = ctx.observe_stats()
        assert (stats["debug_jpeg_commands"], stats["seeded_colour_frames"], stats["colour_commands"]) == (0, 0, 0)
    assert runs[0] == runs[1]
    assert np.frombuffer(runs[1][0][-1][0][:64], np.uint32)[14] == 0


def test_refusals_leave_the_queue_untouched(world):
    """A wrong count, seeds with debug images on, seeds after a ticket, another number of streams with seeds installed: each
    VSF_ERR_INVALID_ARG and followed by a valid frame whose result is what it would have been.  Without the seeds call the
    three switches still return VSF_ERR_UNSUPPORTED with three streams."""
    from vision_slam_frontend_amd import capi
    frames, calibs, want = world
    INV, UNS = capi.VSF_ERR_INVALID_ARG, capi.VSF_ERR_UNSUPPORTED
    L = capi.lib()
    nxt = [0, 0, 0]

    def valid(ctx, s, debug=True):
        left, right = frames[s][nxt[s]]
        t = ctx.observe_submit_stream(s, left, right, calibs[s], best_percent=ts.BPS[s], frame_life=LIFE)
        got = (ctx.observe_collect_bytes(t, LIFE)[1].tobytes(),) + (_pics(ctx, None, t) if debug else ())
        nxt[s] += 1
        return got

    with ts._queue(8, 8) as ctx:
        assert ctx.observe_set_debug_seeds(SEEDS[:2], allow_status=(INV,)) == INV  # n != n_streams
        assert ctx.observe_set_debug_seeds(SEEDS + [9], allow_status=(INV,)) == INV
        for call, arg in ((L.vsf_observe_set_debug_images, 1), (L.vsf_observe_set_debug_jpeg, 90), (L.vsf_observe_set_debug_png, 1)):
            assert call(ctx._h, arg) == UNS  # (the refused calls installed nothing)
        ctx.observe_set_debug_seeds(SEEDS)
        _switch(ctx, None)
        assert ctx.observe_set_debug_seeds([3, 3, 3], allow_status=(INV,)) == INV  # debug images are on
        assert ctx.observe_set_debug_seeds(None, allow_status=(INV,)) == INV
        for n in (1, 2, 4):
            assert ctx.observe_set_streams(n, allow_status=(INV,)) == INV  # another count with seeds installed
        assert ctx.observe_set_streams(3) == capi.VSF_OK
        for s in (0, 1, 2, 1, 0):
            k = nxt[s]
            assert valid(ctx, s) == want[s][k], (s, k)
        assert ctx.observe_set_debug_seeds([3, 3, 3], allow_status=(INV,)) == INV
        assert valid(ctx, 2) == want[2][1]
    # seeds after a ticket, debug images off
    plain = ts._own_context(frames[0][:3], calibs[0], ts.BPS[0])
    nxt[:] = [0, 0, 0]
    with ts._queue(8, 8) as ctx:
        assert valid(ctx, 0, debug=False) == (plain[0],)
        assert ctx.observe_set_debug_seeds(SEEDS, allow_status=(INV,)) == INV
        assert L.vsf_observe_set_debug_images(ctx._h, 1) == UNS  # (nothing was installed)
        assert valid(ctx, 0, debug=False) == (plain[1],)
        ctx.observe_reset()  # ... and after vsf_observe_reset the call is legal again
        ctx.observe_set_debug_seeds(SEEDS)
        _switch(ctx, None)
        nxt[:] = [0, 0, 0]
        assert valid(ctx, 0) == want[0][0]
