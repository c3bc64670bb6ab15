"""vsf_observe_submit_compressed / Frontend::ObserveCompressedImage: sensor_msgs::CompressedImage payloads (JPEG baseline,
with restart intervals, progressive; PNG) go into the ObserveImage queue as they came (the reference's caller,
slam_frontend_main.cc:98-133) and are decoded on the GPU inside the batch.  The yardstick is decode-then-observe: the same
queue fed, through vsf_observe_submit, the images that the system's libjpeg / libpng (tests/jpeg_ref.py, tests/png_ref.py,
driven as cv::imdecode drives them) decode from the same files -- followed, for bayer_rggb8 frames, by the existing
vsf_bayer_bg_to_gray_batch_dev.  Results must be EQUAL BYTE FOR BYTE: both sides run the same extraction and tail on images
the decoder tests already hold bit-exact, so there is no tolerance to choose.

Header word 13 (bytes 52..56 of a result) is the one place where a frame whose file the DEVICE refused differs from the raw
frame it is compared with: it names the refused file (include/vsf.h), so it is asserted on its own and masked in the byte
comparison of THAT ticket only."""
import io
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

W, H, NF, LIFE = 320, 240, 500, 3
F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
GOLD = Path(__file__).resolve().parent / "golden" / "jpeg"
BP = float(np.float32(0.3))


def _refs():
    import jpeg_ref
    import png_ref
    if not (jpeg_ref.available() and png_ref.available()):
        pytest.skip("the system's libjpeg / libpng are not loadable here")
    return jpeg_ref, png_ref


def _encode(img, fmt):
    PIL = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    im = PIL.fromarray(np.ascontiguousarray(img), "L")
    if fmt == "jpeg":
        im.save(b, "JPEG", quality=88)
    elif fmt == "restart":
        im.save(b, "JPEG", quality=82, restart_marker_rows=2)
    elif fmt == "progressive":
        im.save(b, "JPEG", quality=85, progressive=True)
    elif fmt == "png":
        im.save(b, "PNG", compress_level=4)
    else:
        raise ValueError(fmt)
    return b.getvalue()


def _decode(data):
    """What cv::imdecode(IMREAD_GRAYSCALE) returns for `data`, by the real libjpeg / libpng."""
    jpeg_ref, png_ref = _refs()
    if data[:4] == b"\x89PNG":
        st, img, _ = png_ref.imdecode_gray(data, W, H)
    else:
        st, img, _ = jpeg_ref.imdecode_gray(data, W, H)
    assert st == 0 and img.shape == (H, W), st
    return img


def _scene_frames(n):
    from vision_slam_frontend_amd import synth
    sc = synth.Scene(W, H, n_objects=400)
    return [(sc.render(f, 0), sc.render(f, 1)) for f in range(n)]


def _calib():
    from vision_slam_frontend_amd import frontend
    return frontend.default_calibration().set("fundamental", F_RECT)


def _context(depth, min_batch=0):
    from vision_slam_frontend_amd import capi
    ctx = capi.Context(capi.default_params(W, H, max_images=2 * min(depth, 16), nfeatures=NF))
    ctx.observe_configure(depth=depth, min_batch=min_batch)
    return ctx


def _demosaic(mosaics):
    """vsf_bayer_bg_to_gray_batch_dev (the existing entry point) over host mosaics [n][H][W]."""
    import torch

    from vision_slam_frontend_amd import capi
    src = torch.from_numpy(np.ascontiguousarray(mosaics)).to("cuda:0")
    dst = torch.zeros_like(src)
    torch.cuda.synchronize()
    with capi.Context(capi.default_params(W, H, max_images=2, nfeatures=100)) as c:
        st = capi.lib().vsf_bayer_bg_to_gray_batch_dev(c._h, src.data_ptr(), len(mosaics), W, H, W * H, W, dst.data_ptr(), W * H, W)
        assert st == capi.VSF_OK and c.sync() == capi.VSF_OK
    return dst.cpu().numpy()


def _run(spec, depth, bayer=False, min_batch=0, allow=()):
    """spec: [("raw", left image, right image) | ("cmp", left file, right file) | ("bay", ...: files of bayer_rggb8 mosaics)];
    `bayer` makes every "cmp" frame a "bay" one.  Keeps up to `depth` frames in the queue
    (the window crosses batch boundaries), collects in order; returns [(status, result bytes)], the queue's stats."""
    calib = _calib()
    out, tickets = [], []
    with _context(depth, min_batch) as ctx:
        for kind, left, right in spec:
            if len(tickets) == depth:
                out.append(ctx.observe_collect_bytes(tickets.pop(0), LIFE, allow_status=allow))
            if kind == "raw":
                tickets.append(ctx.observe_submit(left, right, calib, best_percent=BP, frame_life=LIFE))
            else:
                st, t = ctx.observe_submit_compressed(left, right, calib, bayer=bayer or kind == "bay", best_percent=BP,
                                                      frame_life=LIFE)
                assert t >= 0
                tickets.append(t)
        while tickets:
            out.append(ctx.observe_collect_bytes(tickets.pop(0), LIFE, allow_status=allow))
        stats = ctx.observe_stats()
    return out, stats


def _reference_spec(spec, bayer):
    ref = []
    for kind, left, right in spec:
        if kind != "raw":
            left, right = _decode(left), _decode(right)
            if bayer or kind == "bay":
                left, right = _demosaic(np.stack([left, right]))
        ref.append(("raw", left, right))
    return ref


def _assert_equal_runs(got, want):
    assert len(got) == len(want)
    for i, ((sa, a), (sb, b)) in enumerate(zip(got, want)):
        assert sa == sb, (i, sa, sb)
        assert a.tobytes() == b.tobytes(), "frame %d differs" % i


FORMATS = {
    "baseline": lambda i: ("jpeg", "jpeg"),
    "restart": lambda i: ("restart", "restart"),
    "progressive": lambda i: ("progressive", "progressive"),
    "png": lambda i: ("png", "png"),
    # every format, left and right of one frame in different formats, and raw frames in between
    "mixed": lambda i: [("jpeg", "png"), ("restart", "restart"), None, ("progressive", "jpeg"), ("png", "png"),
                        ("png", "restart"), None][i % 7],
}


def _spec(case, n=13):
    spec = []
    for i, (left, right) in enumerate(_scene_frames(n)):
        fmt = FORMATS[case](i)
        spec.append(("raw", left, right) if fmt is None else ("cmp", _encode(left, fmt[0]), _encode(right, fmt[1])))
    if case == "mixed":  # the committed 320x240 fixtures join as a frame of their own (baseline left, progressive right)
        spec.insert(5, ("cmp", (GOLD / "gray_320x240_q80.jpg").read_bytes(), (GOLD / "prog_gray_320x240_q85.jpg").read_bytes()))
    return spec


@pytest.mark.parametrize("depth", [1, 4, 32])
@pytest.mark.parametrize("case", list(FORMATS))
def test_compressed_frames_equal_decode_then_observe(case, depth):
    """1. 13-14 stereo frames per case; queue depths 1 (batches of one), 4 (partial batches at the ends) and 32 (capped at 16
    frames per batch here: a full batch); the window of `depth` frames in flight crosses batch boundaries."""
    spec = _spec(case)
    got, stats = _run(spec, depth)
    want, _ = _run(_reference_spec(spec, False), depth)
    _assert_equal_runs(got, want)
    assert stats["compressed"] == sum(k == "cmp" for k, _, _ in spec) and stats["frames"] == len(spec)
    assert stats["ingest_commands"] >= 3 * (stats["batches"] if case != "mixed" else 1) and stats["compressed_bytes"] > 0
    assert all(int(b[52:56].view(np.uint32)[0]) == 0 for _, b in got)


@pytest.mark.parametrize("depth", [1, 4, 32])
def test_bayer_frames_equal_decode_demosaic_then_observe(depth):
    """1. with bayer_rggb8: the decoded image is a mosaic (JPEG and PNG frames alternate); COLOR_BayerBG2BGR + COLOR_BGR2GRAY
    inside the batch against vsf_bayer_bg_to_gray_batch_dev on libjpeg's / libpng's images."""
    spec = []
    for i, (left, right) in enumerate(_scene_frames(12)):
        fmt = ("jpeg", "png", "progressive", "restart")[i % 4]
        spec.append(("cmp", _encode(left, fmt), _encode(right, fmt)))
    got, _ = _run(spec, depth, bayer=True)
    want, _ = _run(_reference_spec(spec, True), depth)
    _assert_equal_runs(got, want)
    plain, _ = _run(spec[:2], depth, bayer=False)
    assert plain[0][1].tobytes() != got[0][1].tobytes()  # (the demosaic did run: the mosaic read as gray gives another frame)


def _cut_png(img):
    import png_craft as pc
    import png_ref
    good = pc.gray8(img)
    s = pc.idat_stream(good)
    bad = pc.replace_idat(good, s[:len(s) // 2])
    assert png_ref.imdecode_gray(bad, W, H)[0] == 2  # libpng: png_error while reading the rows
    return bad


def _cut_restart_jpeg(img):
    """A progressive JPEG with restart intervals, cut inside its last scan (every scan header has been seen, so the host
    accepts it): the decoder looks for the next restart marker and the data have run out."""
    PIL = pytest.importorskip("PIL.Image")
    b = io.BytesIO()
    PIL.fromarray(np.ascontiguousarray(img), "L").save(b, "JPEG", quality=85, progressive=True, restart_marker_rows=2)
    data = b.getvalue()
    sos = data.rfind(b"\xFF\xDA")  # (0xFF 0xDA cannot occur inside entropy-coded data)
    assert data.count(b"\xFF\xDA") > 3 and sos > 0
    return data[:sos + (len(data) - sos) // 2]


@pytest.mark.parametrize("damage,which", [("png_idat_cut", "left"), ("jpeg_cut_inside_scan", "left"),
                                          ("png_idat_cut", "right"), ("jpeg_cut_inside_scan", "both")])
def test_a_file_the_device_refuses_becomes_a_zero_image_for_its_ticket_only(damage, which):
    """2. The LEFT image of frame 3 of a batch of 8 (the issue's two cases) -- and, beyond them, the RIGHT image, and both
    files of the frame (left the cut JPEG, right the cut PNG).  That ticket's collect returns VSF_ERR_INVALID_ARG and header
    word 13 says bit 0 (left) / bit 1 (right); all 8 results equal the raw path's with that image replaced by zeros -- frame 4 included, whose
    threshold is the NaN frame 3 left behind.  (The JPEG is a progressive one with restart intervals: a stream that merely
    ends early is read like libjpeg reads it and is NOT refused -- tests/test_gpu_jpeg.py -- a scan that breaks off where its
    next restart marker should be is, which is what sets bit 1 of vsf_sync's status after vsf_jpeg_decode_gray_batch.)"""
    from vision_slam_frontend_amd import capi
    _refs()
    frames = _scene_frames(8)
    spec = [("cmp", _encode(left, "png" if i & 1 else "jpeg"), _encode(right, "jpeg")) for i, (left, right) in enumerate(frames)]
    cut = _cut_png if damage == "png_idat_cut" else _cut_restart_jpeg
    zero = np.zeros((H, W), np.uint8)
    if which == "left":
        spec[3], ref3, word = ("cmp", cut(frames[3][0]), spec[3][2]), ("raw", zero, _decode(spec[3][2])), 1
    elif which == "right":
        spec[3], ref3, word = ("cmp", spec[3][1], cut(frames[3][1])), ("raw", _decode(spec[3][1]), zero), 2
    else:
        spec[3], ref3, word = ("cmp", cut(frames[3][0]), _cut_png(frames[3][1])), ("raw", zero, zero), 3
    got, stats = _run(spec, 8, min_batch=8, allow=(capi.VSF_ERR_INVALID_ARG,))
    assert stats["max_batch"] == 8 and stats["batches"] == 1
    ref = _reference_spec(spec[:3], False) + [ref3] + _reference_spec(spec[4:], False)
    want, _ = _run(ref, 8, min_batch=8)
    assert [s for s, _ in got] == [capi.VSF_OK] * 3 + [capi.VSF_ERR_INVALID_ARG] + [capi.VSF_OK] * 4
    assert [int(b[52:56].view(np.uint32)[0]) for _, b in got] == [0, 0, 0, word, 0, 0, 0, 0]
    for i, ((_, a), (_, b)) in enumerate(zip(got, want)):
        a = a.copy()
        a[52:56] = 0
        assert a.tobytes() == b.tobytes(), "frame %d differs" % i
    hdr3, hdr4 = got[3][1][:64].view(np.uint32), got[4][1][:64]
    assert hdr3[2] == 0 and hdr3[4 if which != "right" else 5] == 0  # no features, no keypoints in the zero image
    assert np.isnan(hdr4.view(np.float32)[9])  # the threshold applied to frame 4 (quirk Q3)


def test_a_baseline_jpeg_that_ends_early_is_not_refused():
    """2b. The ordinary "JPEG cut inside its scan": a baseline file without restart intervals whose data simply end.  The
    decoders read it as libjpeg reads it (zero bits, a warning, an image), so through the queue it is a frame like any other:
    VSF_OK, word 13 == 0, and the result of decode-then-observe on libjpeg's image."""
    _refs()
    frames = _scene_frames(6)
    spec = [("cmp", _encode(left, "jpeg"), _encode(right, "jpeg")) for left, right in frames]
    whole = spec[2][1]
    sos = whole.find(b"\xFF\xDA")
    spec[2] = ("cmp", whole[:sos + (len(whole) - sos) // 2], spec[2][2])
    assert not np.array_equal(_decode(spec[2][1]), _decode(whole))  # (the lower part of the image is gone)
    got, _ = _run(spec, 4)
    want, _ = _run(_reference_spec(spec, False), 4)
    _assert_equal_runs(got, want)
    assert all(int(b[52:56].view(np.uint32)[0]) == 0 for _, b in got)


def test_frames_with_different_bayer_never_share_a_batch():
    """Bayer and plain compressed frames and raw frames submitted back to back into one queue of depth 8, nothing collected
    in between (so all of them WAIT together and only the submit-side rule separates them): every frame is decoded the way
    its own flag says -- decode(-demosaic)-then-observe frame by frame -- and the batches are cut where the flag changes."""
    frames = _scene_frames(8)
    kinds = ["bay", "bay", "cmp", "cmp", "raw", "bay", "bay", "cmp"]
    fmts = ["jpeg", "png", "png", "jpeg", None, "progressive", "jpeg", "restart"]
    spec = [("raw", left, right) if k == "raw" else (k, _encode(left, f), _encode(right, f))
            for k, f, (left, right) in zip(kinds, fmts, frames)]
    got, stats = _run(spec, 8, min_batch=8)
    want, _ = _run(_reference_spec(spec, False), 8, min_batch=8)
    _assert_equal_runs(got, want)
    # bay bay | cmp cmp raw | bay bay | cmp: a change of the flag sends what waits (raw frames count as not-Bayer)
    assert stats["batches"] == 4 and stats["max_batch"] == 3, stats
    wrong, _ = _run([("cmp",) + spec[0][1:], spec[1]], 8, min_batch=8)
    assert wrong[0][1].tobytes() != got[0][1].tobytes()  # (the flag matters: the same file read as gray is another frame)


@pytest.mark.parametrize("pipelined", [False, True])
def test_frontend_books_a_device_refused_frame_as_a_node_without_features(pipelined):
    """4b. The cut PNG of check 2 as the LEFT payload of frame 3 of an 8-frame drive through Frontend::ObserveCompressedImage:
    the problem equals ObserveImage's on the decoded images with that image all zero (node 3 has no features, the window and
    the threshold chain go on), refused_frames() counts the frame once it is booked and stays; in synchronous mode
    last_status reads VSF_ERR_INVALID_ARG right after that call."""
    from vision_slam_frontend_amd import capi, frontend
    _refs()
    frames = _scene_frames(8)
    files = [(_encode(left, "jpeg"), _encode(right, "png")) for left, right in frames]
    files[3] = (_cut_png(frames[3][0]), files[3][1])
    q = np.array([1, 0, 0, 0], np.float32)
    runs = []
    for compressed in (True, False):
        fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, frame_life=LIFE)
        fe.set_pipelined(pipelined)
        fe.observe_odometry([0, 0, 0], q, 0.0)
        for f, (left, right) in enumerate(files):
            fe.observe_odometry([0.3 * (f + 1), 0, 0], q, 1.0 + f)
            if compressed:
                assert fe.observe_compressed_image(left, right, allow_status=(capi.VSF_ERR_INVALID_ARG,)) is True
                if not pipelined:
                    assert fe.last_status == (capi.VSF_ERR_INVALID_ARG if f == 3 else capi.VSF_OK)
                    assert fe.refused_frames == (1 if f >= 3 else 0)
            else:
                assert fe.observe_image(np.zeros((H, W), np.uint8) if f == 3 else _decode(left), _decode(right)) is True
        assert fe.flush()
        assert fe.refused_frames == (1 if compressed else 0)
        assert fe.last_status == capi.VSF_OK  # (the frames booked after it brought their own status: the counter is what stays)
        runs.append(dict(nodes=fe.nodes(), factors=fe.vision_factors(), wire=fe.serialize_problem()))
        fe.close()
    a, b = runs
    assert len(a["nodes"]) == len(b["nodes"]) == 8 and len(a["nodes"][3]["features"]) == 0 and len(a["nodes"][2]["features"]) > 20
    for na, nb in zip(a["nodes"], b["nodes"]):
        assert na["features"].tobytes() == nb["features"].tobytes()
    assert len(a["factors"]) == len(b["factors"])
    for (a0, a1, ap), (b0, b1, bp) in zip(a["factors"], b["factors"]):
        assert (a0, a1) == (b0, b1)
        np.testing.assert_array_equal(ap, bp)
    assert a["wire"] == b["wire"]


def test_a_file_the_host_refuses_books_nothing():
    """3. A broken header, another size, not an image, above the byte cap: the submit returns the decoder's status and no
    ticket, and the frames around it are those of a run in which that submit never happened."""
    from vision_slam_frontend_amd import capi
    _refs()
    frames = _scene_frames(6)
    files = [(_encode(left, "jpeg"), _encode(right, "png")) for left, right in frames]
    calib = _calib()
    refused = [
        (files[2][0][:100], capi.VSF_ERR_INVALID_ARG),                                   # cut inside the headers
        ((GOLD / "gray_160x120_optimized.jpg").read_bytes(), capi.VSF_ERR_INVALID_ARG),  # another size
        (b"BM" + bytes(200), capi.VSF_ERR_UNSUPPORTED),                                  # neither JPEG nor PNG
        (files[2][1][:30], capi.VSF_ERR_INVALID_ARG),                                    # a PNG cut inside IHDR
    ]
    got = []
    with _context(4) as ctx:
        tickets = []
        for i, (left, right) in enumerate(files):
            if i == 2:
                for k, (bad, want_status) in enumerate(refused):
                    args = (bad, right) if k & 1 == 0 else (left, bad)
                    st, t = ctx.observe_submit_compressed(*args, calib, best_percent=BP, frame_life=LIFE,
                                                          allow_status=(want_status,))
                    assert (st, t) == (want_status, -1), (k, st, t)
            if len(tickets) == 4:
                got.append(ctx.observe_collect_bytes(tickets.pop(0), LIFE))
            tickets.append(ctx.observe_submit_compressed(left, right, calib, best_percent=BP, frame_life=LIFE)[1])
        assert tickets == [2, 3, 4, 5]  # no ticket was spent on a refused file
        while tickets:
            got.append(ctx.observe_collect_bytes(tickets.pop(0), LIFE))
        assert ctx.observe_stats()["frames"] == 6
    want, _ = _run([("cmp", left, right) for left, right in files], 4)
    _assert_equal_runs(got, want)
    # the byte cap: a setter of vsf_observe_configure's kind; a larger file fails ITS submit with VSF_ERR_CAPACITY
    with _context(4) as ctx:
        small = min(len(files[0][0]), len(files[0][1])) - 1
        ctx.observe_set_compressed_cap(small)
        st, t = ctx.observe_submit_compressed(*files[0], calib, best_percent=BP, frame_life=LIFE, allow_status=(capi.VSF_ERR_CAPACITY,))
        assert (st, t) == (capi.VSF_ERR_CAPACITY, -1)
        ctx.observe_set_compressed_cap(0)
        st, t = ctx.observe_submit_compressed(*files[0], calib, best_percent=BP, frame_life=LIFE)
        assert (st, t) == (capi.VSF_OK, 0)
        assert ctx.observe_collect_bytes(t, LIFE)[1].tobytes() == want[0][1].tobytes()


@pytest.mark.parametrize("pipelined", [False, True])
def test_frontend_observe_compressed_image_books_the_decoded_problem(pipelined):
    """4. Frontend::ObserveCompressedImage through frontend.py: nodes, vision factors, odometry factors and the serialised
    problem of a 12-frame drive equal ObserveImage's on the decoded images; a frame the odometry gate holds back returns
    false without its (garbage) payload being parsed."""
    from vision_slam_frontend_amd import capi, frontend
    _refs()
    frames = _scene_frames(12)
    fmts = ("jpeg", "png", "progressive", "restart")
    files = [(_encode(left, fmts[i % 4]), _encode(right, fmts[(i + 1) % 4])) for i, (left, right) in enumerate(frames)]
    q = np.array([1, 0, 0, 0], np.float32)
    runs = []
    for compressed in (True, False):
        fe = frontend.Frontend(W, H, nfeatures=NF, fundamental=F_RECT, frame_life=LIFE)
        fe.set_pipelined(pipelined)
        fe.observe_odometry([0, 0, 0], q, 0.0)
        for f, (left, right) in enumerate(files):
            fe.observe_odometry([0.3 * (f + 1), 0, 0], q, 1.0 + f)
            if compressed:
                assert fe.observe_compressed_image(left, right) is True
            else:
                assert fe.observe_image(_decode(left), _decode(right)) is True
            if f % 4 == 1:  # the gate: no motion since the last frame
                fe.observe_odometry([0.3 * (f + 1), 0, 0], q, 1.5 + f)
                if compressed:
                    assert fe.observe_compressed_image(b"garbage", b"more garbage") is False
                    assert fe.last_status == capi.VSF_OK or pipelined  # (not parsed: nothing to refuse)
                else:
                    assert fe.observe_image(_decode(left), _decode(right)) is False
        if compressed:  # a host-refused file: false, the status says why, nothing is booked
            fe.observe_odometry([0.3 * 20, 0, 0], q, 40.0)
            assert fe.observe_compressed_image(files[0][0][:90], files[0][1], allow_status=(capi.VSF_ERR_INVALID_ARG,)) is False
            assert fe.last_status == capi.VSF_ERR_INVALID_ARG
        assert fe.flush()
        runs.append(dict(nodes=fe.nodes(), factors=fe.vision_factors(), odo=fe.odometry_factors(), wire=fe.serialize_problem()))
        fe.close()
    a, b = runs
    assert len(a["nodes"]) == len(b["nodes"]) == 12
    for na, nb in zip(a["nodes"], b["nodes"]):
        assert na["node_idx"] == nb["node_idx"] and na["timestamp"] == nb["timestamp"]
        np.testing.assert_array_equal(na["pose"], nb["pose"])
        assert na["features"].tobytes() == nb["features"].tobytes()
    assert len(a["factors"]) == len(b["factors"]) > 20
    for (a0, a1, ap), (b0, b1, bp) in zip(a["factors"], b["factors"]):
        assert (a0, a1) == (b0, b1)
        np.testing.assert_array_equal(ap, bp)
    assert len(a["odo"]) == len(b["odo"]) == 11
    assert a["wire"] == b["wire"]


# What the commit before compressed frames existed reports for the raw run of check 5 below: its library, built from that
# commit and run on an MI355X beside this one, gave these launches per profiled stage (vsf_profile_read's second value: a
# count, no time) and these queue counters.  They are what "unchanged" means here; a change of the raw path's launches has to
# change them on purpose.
PARENT_LAUNCHES = {"pyramid_resize": 196, "fast_score_nms": 4, "select_harris_angle": 4, "gauss_blur7": 4, "orb_describe": 4,
                   "hamming_knn2": 8, "ratio_compact": 8, "frontend_tail": 24}
PARENT_STATS = dict(frames=13, batches=4, max_batch=4, solo=1, forced=1, slot_waits=0, depth=4, bmax=4)


def _raw_run(ctx, frames, calib):
    ctx.observe_configure(depth=4, min_batch=4)
    ctx.profile_enable(True)
    results = []
    for i0 in range(0, 13, 4):
        tickets = [ctx.observe_submit(left, right, calib, best_percent=BP, frame_life=LIFE) for left, right in frames[i0:i0 + 4]]
        results += [ctx.observe_collect_bytes(t, LIFE) for t in tickets]
    launches = {k: n for k, (_, n) in ctx.profile_read().items()}
    return results, launches, ctx.observe_stats()


def test_raw_only_queue_counts_are_unchanged():
    """5. Only raw frames (13 frames at depth 4, min_batch 4, submitted four at a time: three batches of 4 and a forced lone
    frame that runs on one stream): the queue's counters AND the launches of every profiled stage are the parent commit's
    (PARENT_*), the compressed path has issued no copy command and no launch (`ingest_commands`: ingest_batch counts every one
    it issues, the ingest finish included) and owns no byte (`compressed_bytes`: file ring, blobs, decoder scratch, mosaics),
    and header word 13 stays 0.  The same holds for a raw run on a context that HAS seen compressed frames, after a reset:
    the same launches per stage, no further command of the compressed path, the same results."""
    from vision_slam_frontend_amd import capi
    calib = _calib()
    frames = _scene_frames(13)
    with capi.Context(capi.default_params(W, H, max_images=8, nfeatures=NF)) as ctx:
        results, launches, s = _raw_run(ctx, frames, calib)
    assert launches == PARENT_LAUNCHES
    assert {k: s[k] for k in PARENT_STATS} == PARENT_STATS
    assert (s["compressed"], s["ingest_commands"], s["compressed_bytes"]) == (0, 0, 0)
    assert all(int(b[52:56].view(np.uint32)[0]) == 0 for _, b in results)
    with capi.Context(capi.default_params(W, H, max_images=8, nfeatures=NF)) as ctx:
        ctx.observe_configure(depth=4, min_batch=4)
        ctx.observe_stereo_compressed(_encode(frames[0][0], "jpeg"), _encode(frames[0][1], "png"), calib, best_percent=BP,
                                      frame_life=LIFE)
        before = ctx.observe_stats()
        assert before["ingest_commands"] == 4 and before["compressed_bytes"] > 0  # (the counters are live: copy, 2 runs, finish)
        ctx.observe_reset()
        again, launches2, s2 = _raw_run(ctx, frames, calib)
    assert launches2 == PARENT_LAUNCHES and s2["ingest_commands"] == 0 and s2["compressed"] == 0
    assert [b.tobytes() for _, b in again] == [b.tobytes() for _, b in results]
