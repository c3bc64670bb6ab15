"""Detection masks in the ObserveImage queue (vsf_observe_set_stream_masks).  The reference throughout is the synchronous
vsf_observe_stereo on a fresh context whose slots vsf_set_image_masks names -- fed only that stream's frames --, and every
collected result is compared whole, header words included: there is no tolerance to choose.  (That the masked extraction
itself is OpenCV's is tests/test_gpu_mask.py's business.)

1. three streams through one queue at depths 1 / 4 / 32: two with different mask pairs (one of them masks the left eye only),
   one without; the stream without is also what a context that never heard of masks returns;
2. the streams really share batches;
3. a stream's slots are changed between two submits, and a slot's mask is replaced between two submits (vsf_mask_set flushes
   inside): frames submitted before keep what they were submitted with;
4. a stream with a declared input size: the mask is at the context's size;
5. one JPEG submit and one Bayer submit."""
import ctypes as C
import io
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import orb_mask_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, NF, LIFE, N = 320, 240, 500, 3, 5
F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
BP = float(np.float32(0.3))
MASKS = ref.masks(W, H)
# per stream: (left mask, right mask) by name, None: no mask
STREAM_MASKS = [("half_plane", "disc"), ("rectangle_two_borders", None), (None, None)]


def _calib():
    from vision_slam_frontend_amd import frontend
    return frontend.default_calibration().set("fundamental", F_RECT)


def _params(batch, w=W, h=H):
    from vision_slam_frontend_amd import capi
    return capi.default_params(w, h, max_images=2 * batch, nfeatures=NF)


def _frames(n_streams=3, w=W, h=H, objects=400):
    from vision_slam_frontend_amd import synth
    out = []
    for s in range(n_streams):
        sc = synth.Scene(w, h, n_objects=objects, seed=synth.BASE_SEED + 29 * s)
        out.append([(sc.render(f, 0), sc.render(f, 1)) for f in range(N)])
    return out


def _sync_bytes(ctx, left, right, calib):
    from vision_slam_frontend_amd import capi
    cap = int(capi.lib().vsf_observe_capacity(ctx._h, LIFE))
    buf, n = np.zeros(cap, np.uint8), C.c_size_t()
    st = capi.lib().vsf_observe_stereo(ctx._h, left.ctypes.data, right.ctypes.data, W, H, left.strides[0], C.byref(calib), BP,
                                       LIFE, buf.ctypes.data, cap, C.byref(n))
    assert st == capi.VSF_OK, st
    return buf[:n.value].tobytes()


def _own_context(frames, calib, masks_at):
    """THE reference: a fresh context fed `frames` through vsf_observe_stereo; masks_at(k) -> (left, right) mask arrays (or
    None) in force for frame k, set through vsf_mask_set / vsf_set_image_masks."""
    from vision_slam_frontend_amd import capi
    out = []
    with capi.Context(_params(1)) as ctx:
        for k, (left, right) in enumerate(frames):
            slots = []
            for side, m in enumerate(masks_at(k)):
                if m is None:
                    slots.append(-1)
                else:
                    ctx.mask_set(10 + side, m)
                    slots.append(10 + side)
            ctx.set_image_masks(*slots)
            out.append(_sync_bytes(ctx, left, right, calib))
    return out


def _pair(names):
    return tuple(None if n is None else MASKS[n] for n in names)


@pytest.fixture(scope="module")
def world():
    """Three sequences and each stream's reference results with its masks (computed once, shared, never changed); the
    unmasked results of stream 0, to show that its masks matter."""
    frames, calib = _frames(), _calib()
    want = [_own_context(frames[s], calib, lambda k, s=s: _pair(STREAM_MASKS[s])) for s in range(3)]
    plain0 = _own_context(frames[0], calib, lambda k: (None, None))
    assert all(a != b for a, b in zip(want[0], plain0))
    for s in range(3):  # not trivial: features, a full window, temporal factors
        hdr = np.frombuffer(want[s][-1][:64], np.uint32)
        assert hdr[1] == LIFE + 1 and hdr[2] > 4, (s, hdr)
    return frames, calib, want, plain0


def _queue(depth, batch, min_batch=0, n_streams=3, set_masks=True):
    from vision_slam_frontend_amd import capi
    ctx = capi.Context(_params(batch))
    ctx.observe_configure(depth, min_batch, 0)
    ctx.observe_set_streams(n_streams)
    if set_masks:
        slot = 0
        for s, names in enumerate(STREAM_MASKS[:n_streams]):
            slots = []
            for name in names:
                if name is None:
                    slots.append(-1)
                else:
                    ctx.mask_set(slot, MASKS[name])
                    slots.append(slot)
                    slot += 1
            ctx.observe_set_stream_masks(s, *slots)
    return ctx


def _drive(ctx, depth, order, frames, calib, submit=None, before=None):
    got, tickets, nxt = [[] for _ in frames], [], [0] * len(frames)
    for s in order:
        if len(tickets) == depth:
            t, sc = tickets.pop(0)
            got[sc].append(ctx.observe_collect_bytes(t, LIFE)[1].tobytes())
        k = nxt[s]
        nxt[s] += 1
        if before:
            before(s, k)
        left, right = frames[s][k]
        t = submit(s, left, right) if submit else ctx.observe_submit_stream(s, left, right, calib, best_percent=BP, frame_life=LIFE)
        tickets.append((t, s))
    for t, sc in tickets:
        got[sc].append(ctx.observe_collect_bytes(t, LIFE)[1].tobytes())
    return got


def _assert_equal(got, want, what="stream"):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, "%s: frame %d differs from its own context's" % (what, k)


ROUND_ROBIN = [s for _ in range(N) for s in range(3)]


# ---- 1 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [1, 4, 32])
def test_streams_with_and_without_masks(world, depth):
    frames, calib, want, _ = world
    with _queue(depth, min(depth, 16)) as ctx:
        got = _drive(ctx, depth, ROUND_ROBIN, frames, calib)
    for s in range(3):
        _assert_equal(got[s], want[s], "depth %d stream %d" % (depth, s))


def test_stream_without_masks_equals_a_context_that_never_heard_of_them(world):
    frames, calib, want, _ = world
    with _queue(4, 4, n_streams=1, set_masks=False) as ctx:
        got = _drive(ctx, 4, [0] * N, [frames[2]], calib)
    _assert_equal(got[0], want[2], "no masks anywhere")


# ---- 2 ----------------------------------------------------------------------------------------------------------------

def test_masked_and_unmasked_streams_share_batches(world):
    frames, calib, want, _ = world
    with _queue(32, 16, min_batch=32) as ctx:  # (nothing leaves until the first collect sends everything)
        got = _drive(ctx, 32, ROUND_ROBIN, frames, calib)
        stats = ctx.observe_stats()
    for s in range(3):
        _assert_equal(got[s], want[s], "stream %d" % s)
    assert stats["batches"] == 1 and stats["max_batch"] == 3 * N and stats["multi_stream_batches"] == 1, stats


# ---- 3 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["other_slots", "slot_replaced"])
def test_mask_changed_between_two_submits(world, how):
    frames, calib, _, _ = world
    first, second = _pair(("half_plane", "disc")), _pair(("disc", "rectangle_two_borders"))
    want = _own_context(frames[0], calib, lambda k: first if k < 2 else second)
    assert want != _own_context(frames[0], calib, lambda k: first)
    with _queue(32, 16, min_batch=32, n_streams=1, set_masks=False) as ctx:
        ctx.mask_set(0, first[0])
        ctx.mask_set(1, first[1])
        ctx.mask_set(2, second[0])
        ctx.mask_set(3, second[1])
        ctx.observe_set_stream_masks(0, 0, 1)

        def before(s, k):
            if k != 2:
                return
            if how == "other_slots":
                ctx.observe_set_stream_masks(0, 2, 3)  # (frames 0 and 1 still wait: they keep slots 0 and 1)
            else:
                ctx.mask_set(0, second[0])  # flushes inside: frames 0 and 1 leave with the slots as they were
                ctx.mask_set(1, second[1])

        got = _drive(ctx, 32, [0] * N, [frames[0]], calib, before=before)
        stats = ctx.observe_stats()
    _assert_equal(got[0], want, how)
    assert stats["batches"] == (1 if how == "other_slots" else 2), stats


# ---- 4 ----------------------------------------------------------------------------------------------------------------

def test_declared_input_size_takes_the_mask_at_the_contexts_size(world):
    from oracle import binding as ob
    _, calib, _, _ = world
    big = _frames(1, 640, 480, objects=1600)[0]
    small = [(ob.resize_linear(l, W, H), ob.resize_linear(r, W, H)) for l, r in big]
    pair = _pair(STREAM_MASKS[0])
    want = _own_context(small, calib, lambda k: pair)
    assert want != _own_context(small, calib, lambda k: (None, None))
    with _queue(4, 4, n_streams=1) as ctx:
        ctx.observe_set_input_size(0, 640, 480)
        got = _drive(ctx, 4, [0] * N, [big], calib,
                     submit=lambda s, l, r: ctx.observe_submit(l, r, calib, best_percent=BP, frame_life=LIFE))
        assert ctx.observe_stats()["resized_frames"] == N
    _assert_equal(got[0], want, "640 x 480 into 320 x 240")


# ---- 5 ----------------------------------------------------------------------------------------------------------------

def test_jpeg_and_bayer_submits(world):
    from oracle import binding as ob
    from vision_slam_frontend_amd import capi
    PIL = pytest.importorskip("PIL.Image")
    frames, calib, _, _ = world
    pair = _pair(STREAM_MASKS[0])

    def jpeg(img):
        b = io.BytesIO()
        PIL.fromarray(np.ascontiguousarray(img), "L").save(b, "JPEG", quality=88)
        return b.getvalue()

    left, right = frames[0][0]
    files = (jpeg(left), jpeg(right))
    mosaics = frames[1][0]  # (any bytes are a mosaic)
    grays = (ob.bayer_bg_to_gray(mosaics[0]), ob.bayer_bg_to_gray(mosaics[1]))
    # the reference: the synchronous calls on a context whose slots vsf_set_image_masks names -- and without masks
    with capi.Context(_params(1)) as ctx:
        plain_jpeg = ctx.observe_stereo_compressed(*files, calib, best_percent=BP, frame_life=LIFE)
    with capi.Context(_params(1)) as ctx:
        ctx.mask_set(0, pair[0])
        ctx.mask_set(1, pair[1])
        ctx.set_image_masks(0, 1)
        want_jpeg = ctx.observe_stereo_compressed(*files, calib, best_percent=BP, frame_life=LIFE)
        want_bayer = _sync_bytes(ctx, grays[0], grays[1], calib)
    assert want_jpeg["keypoints"].tobytes() != plain_jpeg["keypoints"].tobytes()
    with _queue(4, 4, n_streams=1) as ctx:
        st, t0 = ctx.observe_submit_compressed_stream(0, *files, calib, best_percent=BP, frame_life=LIFE)
        assert st == capi.VSF_OK
        t1 = ctx.observe_submit_stream_pix(0, mosaics[0], mosaics[1], capi.PIX_BAYER_RGGB8, calib, best_percent=BP, frame_life=LIFE)
        got_jpeg = capi.decode_observation(ctx.observe_collect_bytes(t0, LIFE)[1])
        got_bayer = ctx.observe_collect_bytes(t1, LIFE)[1].tobytes()
    for key in ("keypoints", "descriptors", "features"):
        assert np.asarray(got_jpeg[key]).tobytes() == np.asarray(want_jpeg[key]).tobytes(), "JPEG frame: " + key
    assert got_bayer == want_bayer, "the Bayer frame differs from the masked synchronous call on its gray images"
