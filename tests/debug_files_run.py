"""What tests/test_gpu_debug_jpeg.py, test_gpu_debug_png.py and test_gpu_encode_path.py share: the frames they submit and ONE run of
them through the ObserveImage queue with the debug images leaving as raw canvases or as files of one form."""
import ctypes as C

import numpy as np

W, H, NF, LIFE, SEED = 320, 240, 500, 3, 11
F_RECT = np.float32([0, 0, 0, 0, 0, -1, 0, 1, 0])
FORMS = ("jpeg", "png")


def make_frames():
    from vision_slam_frontend_amd import synth
    sc = synth.Scene(W, H)
    fr = [(sc.render(f, 0), sc.render(f, 1)) for f in range(5)]
    fr[2] = (fr[2][0], np.zeros_like(fr[2][1]))  # an empty right image: no stereo match, so no stereo image for this frame
    return fr


def seed(ctx):
    """The stereo lines' colours come from the process's rand(), drawn at submit: seeded once the context exists (the HIP runtime's
    own start-up, which the first context of a process triggers, does not leave rand() where it was)."""
    from vision_slam_frontend_amd import capi
    assert ctx.sync() == capi.VSF_OK
    C.CDLL("libc.so.6").srand(SEED)


def files_view(ctx, form, ticket):
    """vsf_observe_debug_<form>_view -> (status, stereo file or None, match file or None)."""
    from vision_slam_frontend_amd import capi
    s_, m_, sn, mn = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    view = getattr(capi.lib(), "vsf_observe_debug_%s_view" % form)
    st = view(ctx._h, ticket, C.byref(s_), C.byref(sn), C.byref(m_), C.byref(mn))
    if st != capi.VSF_OK:
        return st, None, None
    assert bool(s_.value) == (sn.value > 0) and bool(m_.value) == (mn.value > 0)
    return st, C.string_at(s_.value, sn.value) if s_.value else None, C.string_at(m_.value, mn.value) if m_.value else None


def canvases_view(ctx, ticket):
    """vsf_observe_debug_view -> (status, stereo canvas or None, match canvas or None)."""
    from vision_slam_frontend_amd import capi
    s_, m_ = C.c_void_p(), C.c_void_p()
    st = capi.lib().vsf_observe_debug_view(ctx._h, ticket, C.byref(s_), C.byref(m_))
    if st != capi.VSF_OK:
        return st, None, None
    return (st, np.frombuffer(C.string_at(s_.value, 6 * W * H), np.uint8).reshape(H, 2 * W, 3) if s_.value else None,
            np.frombuffer(C.string_at(m_.value, 3 * W * H), np.uint8).reshape(H, W, 3) if m_.value else None)


def submit_collect(ctx, frames, depth, form):
    """Frames through the queue, `depth` at a time.  form: "jpeg" / "png" = the files are in force, None = the raw canvases, False =
    no debug images.  Every view that is not the one in force must refuse.  -> (results, canvases or files per frame)"""
    from vision_slam_frontend_amd import capi, frontend
    calib = frontend.default_calibration().set("fundamental", F_RECT.reshape(9))
    L = capi.lib()
    cap = L.vsf_observe_capacity(ctx._h, LIFE)
    outs, pics = [], []
    for g0 in range(0, len(frames), depth):
        tickets = []
        for left, right in frames[g0:g0 + depth]:
            t = C.c_int64()
            assert L.vsf_observe_submit(ctx._h, left.ctypes.data, right.ctypes.data, W, H, W, C.byref(calib), C.c_float(0.3),
                                        LIFE, C.byref(t)) == capi.VSF_OK
            tickets.append(t.value)
        for t in tickets:
            buf = np.zeros(cap, np.uint8)
            n = C.c_size_t()
            assert L.vsf_observe_collect(ctx._h, t, buf.ctypes.data, cap, C.byref(n)) == capi.VSF_OK
            outs.append(buf[:n.value].copy())
        for t in tickets:
            if form is False:
                continue
            for other in FORMS:
                if other != form:
                    assert files_view(ctx, other, t)[0] == capi.VSF_ERR_INVALID_ARG
            if form:
                st, s, m = files_view(ctx, form, t)
                assert canvases_view(ctx, t)[0] == capi.VSF_ERR_INVALID_ARG
            else:
                st, s, m = canvases_view(ctx, t)
            assert st == capi.VSF_OK
            pics.append((s, m))
    return outs, pics


def run(frames, depth, images, form, value):
    """One context: vsf_observe_set_debug_images(1) if `images`, then vsf_observe_set_debug_<form>(value) unless value is None (the
    call is never made).  -> (results, raw canvases or files per frame, stats)"""
    from vision_slam_frontend_amd import capi
    L = capi.lib()
    setter = getattr(L, "vsf_observe_set_debug_%s" % form)
    with capi.Context(capi.default_params(W, H, max_images=2 * depth, nfeatures=NF), device=0) as ctx:
        ctx.observe_configure(depth=depth)
        ctx.profile_enable(True)  # (the per-stage launch counts of vsf_profile_read)
        seed(ctx)
        if images:
            assert L.vsf_observe_set_debug_images(ctx._h, 1) == capi.VSF_OK
        if value is not None:
            assert setter(ctx._h, value) == capi.VSF_OK
        outs, pics = submit_collect(ctx, frames, depth, form if value else None if images else False)
        if value:  # the window holds frames: the switch no longer moves
            assert setter(ctx._h, 0) == capi.VSF_ERR_INVALID_ARG
        stats = ctx.observe_stats()
        stats["launches"] = {k: v[1] for k, v in ctx.profile_read().items()}
        return outs, pics, stats
