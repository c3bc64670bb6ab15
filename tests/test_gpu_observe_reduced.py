"""vsf_observe_submit_compressed_reduced: JPEG payloads read as cv::imdecode(IMREAD_REDUCED_GRAYSCALE_2 / _4) reads them go
into the ObserveImage queue and are decoded at 1/2 or 1/4 inside the batch.  The yardstick is decode-then-observe: the same
queue fed, through vsf_observe_submit, the images the system's libjpeg decodes from the same files at the same scale
(tests/jpeg_ref_reduced.py).  Results must be EQUAL BYTE FOR BYTE -- both sides run the same extraction and tail, so there
is no tolerance to choose.  A 64 x 48 context is fed 128 x 96 and 127 x 95 files at 1/2 and 256 x 192 files at 1/4 (the
shapes at which sizes differ below the denominator); a 160 x 120 context fed 320 x 240 files repeats the comparison where
frames carry features, stereo matches and temporal factors."""
import io
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

NF, LIFE = 500, 3
F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
F_SHIFT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 1.5]], np.float32)
BP = float(np.float32(0.3))
TIMES = ("copy_ns", "launch_ns", "wait_ns")  # the host's clocks: the only values of vsf_observe_stats that differ run to run


def _ref():
    import jpeg_ref_reduced as ref
    assert ref.available(), "no libjpeg.so.8 to build tests/cpp/jpeg_ref_reduced.c against"
    return ref


def _jpeg(img, i):
    import PIL.Image as PIL
    b = io.BytesIO()
    kw = [dict(quality=88), dict(quality=82, restart_marker_rows=2), dict(quality=85, progressive=True), dict(quality=93, optimize=True)][i % 4]
    PIL.fromarray(np.ascontiguousarray(img), "L").save(b, "JPEG", **kw)
    return b.getvalue()


def _png(img):
    import PIL.Image as PIL
    b = io.BytesIO()
    PIL.fromarray(np.ascontiguousarray(img), "L").save(b, "PNG")
    return b.getvalue()


def _calib(F=F_RECT):
    from vision_slam_frontend_amd import frontend
    return frontend.default_calibration().set("fundamental", F)


def _context(w, h, depth, streams=1):
    from vision_slam_frontend_amd import capi
    ctx = capi.Context(capi.default_params(w, h, max_images=2 * min(depth, 16), nfeatures=NF))
    ctx.observe_configure(depth=depth)
    ctx.observe_set_compressed_cap(1 << 19)  # (the cap applies to the file as it is: a 640 x 480 file into a 160 x 120 context)
    if streams > 1:
        ctx.observe_set_streams(streams)
    return ctx


def _spec(w, h, n=12):
    """[("raw", left, right, stream) | ("cmp", left file, right file, stream, d)]: files of d x the context's size (one pixel
    less a side every other time at 1/2: they reduce to the same size), full-size compressed frames (d = 1) and raw frames."""
    from vision_slam_frontend_amd import synth
    scenes = {d: synth.Scene(w * d, h * d, n_objects=60 * d * d + 200 * (w > 100), seed=synth.BASE_SEED + d) for d in (1, 2, 4)}
    spec = []
    for i in range(n):
        d = (2, 2, 4, 1, 0, 2, 4, 4, 1, 2, 0, 2)[i % 12]
        if d == 0:
            spec.append(("raw", scenes[1].render(i, 0), scenes[1].render(i, 1), 0))
            continue
        left, right = scenes[d].render(i, 0), scenes[d].render(i, 1)
        if d == 2 and i % 2:
            left, right = left[:h * 2 - 1, :w * 2 - 1], right[:h * 2 - 1, :w * 2 - 1]
        spec.append(("cmp", _jpeg(left, i), _jpeg(right, i + 1), 0, d))
    return spec


def _reference_spec(spec, w, h):
    ref = _ref()
    out = []
    for item in spec:
        if item[0] == "cmp":
            imgs = []
            for f in item[1:3]:
                st, img, warn = ref.imdecode_reduced_gray(f, item[4], w, h)
                assert st == 0 and warn == 0 and img.shape == (h, w)
                imgs.append(img)
            item = ("raw", imgs[0], imgs[1], item[3])
        out.append(item)
    return out


def _run(spec, w, h, depth, streams=1, calibs=None):
    """Keeps up to `depth` frames in the queue, collects in order -> [(status, result bytes)], the queue's stats."""
    from vision_slam_frontend_amd import capi
    calibs = calibs or [_calib()]
    out, tickets = [], []
    with _context(w, h, depth, streams) as ctx:
        for item in spec:
            if len(tickets) == depth:
                out.append(ctx.observe_collect_bytes(tickets.pop(0), LIFE))
            s = item[3]
            if item[0] == "raw":
                t = ctx.observe_submit_stream(s, item[1], item[2], calibs[s], best_percent=BP, frame_life=LIFE)
            elif item[4] == 1 and s == 0 and streams == 1:
                st, t = ctx.observe_submit_compressed(item[1], item[2], calibs[s], best_percent=BP, frame_life=LIFE)
            else:
                st, t = ctx.observe_submit_compressed_reduced(item[1], item[2], calibs[s], item[4], stream=s, best_percent=BP,
                                                              frame_life=LIFE)
            assert t >= 0
            tickets.append(t)
        while tickets:
            out.append(ctx.observe_collect_bytes(tickets.pop(0), LIFE))
        stats = ctx.observe_stats()
    assert all(st == capi.VSF_OK for st, _ in out)
    return [b.tobytes() for _, b in out], stats


@pytest.mark.parametrize("depth", [1, 4, 32])
def test_reduced_full_size_and_raw_frames_in_one_run_of_tickets(depth):
    w, h = 64, 48
    spec = _spec(w, h)
    got, stats = _run(spec, w, h, depth)
    want, _ = _run(_reference_spec(spec, w, h), w, h, depth)
    assert got == want
    n_cmp = sum(i[0] == "cmp" for i in spec)
    assert stats["frames"] == len(spec) and stats["compressed"] == n_cmp
    assert stats["reduced_frames"] == sum(i[0] == "cmp" and i[4] > 1 for i in spec) == 8
    assert all(int(np.frombuffer(b[52:56], np.uint32)[0]) == 0 for b in got)   # no file was refused on the device


def test_frames_with_features_equal_decode_then_observe():
    """The same at 160 x 120 from 320 x 240 / 319 x 239 and 640 x 480 files, where a frame has keypoints, stereo matches, 3-D
    points and temporal factors: a wrong pixel anywhere in a decoded image moves them."""
    w, h = 160, 120
    spec = _spec(w, h, n=8)
    got, stats = _run(spec, w, h, 4)
    want, _ = _run(_reference_spec(spec, w, h), w, h, 4)
    assert got == want
    hdr = np.frombuffer(got[-1][:64], np.uint32)
    assert hdr[1] == LIFE + 1 and hdr[2] > 20 and hdr[6] > 20, hdr   # a full window, features, stereo matches
    assert stats["reduced_frames"] == 6


def test_two_streams_with_different_denominators():
    """Stream 0 brings 128 x 96 files at 1/2, stream 1 brings 256 x 192 files at 1/4 and another calibration; their frames
    share batches (and the batch's one upload).  Against the same two-stream queue fed the library's images raw."""
    from vision_slam_frontend_amd import synth
    w, h = 64, 48
    calibs = [_calib(F_RECT), _calib(F_SHIFT)]
    scenes = [synth.Scene(w * 2, h * 2, n_objects=240, seed=synth.BASE_SEED + 5), synth.Scene(w * 4, h * 4, n_objects=900, seed=synth.BASE_SEED + 6)]
    spec, k = [], [0, 0]
    for s in (0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0):
        f = k[s]
        k[s] += 1
        spec.append(("cmp", _jpeg(scenes[s].render(f, 0), f), _jpeg(scenes[s].render(f, 1), f + 2), s, (2, 4)[s]))
    got, stats = _run(spec, w, h, 8, streams=2, calibs=calibs)
    want, _ = _run(_reference_spec(spec, w, h), w, h, 8, streams=2, calibs=calibs)
    assert got == want
    assert stats["reduced_frames"] == 12 and stats["streams"] == 2 and stats["frames"] == 12


def test_a_host_refused_file_takes_no_ticket_and_changes_nothing():
    from vision_slam_frontend_amd import capi, synth
    w, h = 64, 48
    sc2, sc4 = synth.Scene(128, 96, n_objects=240), synth.Scene(256, 192, n_objects=900)
    frames = [(_jpeg(sc2.render(i, 0), i), _jpeg(sc2.render(i, 1), i)) for i in range(3)]
    big = _jpeg(sc4.render(0, 0), 0)
    png = _png(sc2.render(0, 0))
    calib = _calib()
    every = range(1, 6)

    def run(with_refusals):
        out = []
        with _context(w, h, 4) as ctx:
            for i, (left, right) in enumerate(frames):
                if with_refusals:
                    before = {k: v for k, v in ctx.observe_stats().items() if k not in TIMES}
                    sub = lambda a, b, d: ctx.observe_submit_compressed_reduced(a, b, calib, d, best_percent=BP, frame_life=LIFE,
                                                                                allow_status=every)
                    assert sub(left, big, 2) == (capi.VSF_ERR_INVALID_ARG, -1)      # the right file is 256 x 192: not 64 x 48 at 1/2
                    assert sub(left, right, 4) == (capi.VSF_ERR_INVALID_ARG, -1)    # the wrong denominator for this size
                    assert sub(left, right, 1) == (capi.VSF_ERR_INVALID_ARG, -1)
                    assert sub(png, right, 2) == (capi.VSF_ERR_UNSUPPORTED, -1)     # a PNG at a reduced size
                    assert sub(left, right, 3) == (capi.VSF_ERR_INVALID_ARG, -1)    # not a denominator
                    assert {k: v for k, v in ctx.observe_stats().items() if k not in TIMES} == before
                st, t = ctx.observe_submit_compressed_reduced(left, right, calib, 2, best_percent=BP, frame_life=LIFE)
                assert t == i   # no ticket was spent on a refusal
                out.append(ctx.observe_collect_bytes(t, LIFE)[1].tobytes())
        return out

    assert run(True) == run(False)


def test_old_paths_issue_the_launches_and_copies_they_always_did():
    """vsf_observe_stats of a raw-only queue, of a full-size compressed queue through the old call and through the new call
    at reduce = 1, and of a reduced queue, at depth 1 (every batch one frame): a raw queue has no compressed-path command at
    all; a compressed batch is one copy command, one decode run and the finish -- three -- whichever call or denominator
    brought it; and the counter of reduced frames moves for reduced frames only."""
    from vision_slam_frontend_amd import synth
    w, h = 64, 48
    sc1, sc2 = synth.Scene(w, h, n_objects=60), synth.Scene(2 * w, 2 * h, n_objects=240)
    raw = [("raw", sc1.render(i, 0), sc1.render(i, 1), 0) for i in range(4)]
    full = [("cmp", _jpeg(sc1.render(i, 0), 0), _jpeg(sc1.render(i, 1), 0), 0, 1) for i in range(4)]
    half = [("cmp", _jpeg(sc2.render(i, 0), 0), _jpeg(sc2.render(i, 1), 0), 0, 2) for i in range(4)]
    _, s_raw = _run(raw, w, h, 1)
    assert (s_raw["compressed"], s_raw["ingest_commands"], s_raw["compressed_bytes"], s_raw["reduced_frames"]) == (0, 0, 0, 0)
    assert s_raw["frames"] == s_raw["batches"] == 4
    got_old, s_old = _run(full, w, h, 1)                       # vsf_observe_submit_compressed
    got_new, s_new = _run_new_call(full, w, h)         # vsf_observe_submit_compressed_reduced, reduce = 1
    assert got_old == got_new
    strip = lambda s: {k: v for k, v in s.items() if k not in TIMES}
    assert strip(s_old) == strip(s_new)
    assert (s_old["compressed"], s_old["ingest_commands"], s_old["reduced_frames"]) == (4, 12, 0)
    _, s_half = _run(half, w, h, 1)
    assert (s_half["compressed"], s_half["ingest_commands"], s_half["reduced_frames"]) == (4, 12, 4)


def _run_new_call(spec, w, h):
    """`spec` of full-size compressed frames through vsf_observe_submit_compressed_reduced at reduce = 1, depth 1."""
    out = []
    with _context(w, h, 1) as ctx:
        for item in spec:
            st, t = ctx.observe_submit_compressed_reduced(item[1], item[2], _calib(), 1, best_percent=BP, frame_life=LIFE)
            out.append(ctx.observe_collect_bytes(t, LIFE)[1].tobytes())
        stats = ctx.observe_stats()
    return out, stats
