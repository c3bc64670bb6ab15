"""cv::ORB::FAST_SCORE (vsf_params::score_type 1) on the GPU, bit for bit against tests/orb_score_ref.py -- keypoints as raw
bytes, descriptors and counts, no tolerance anywhere.  (tests/test_orb_score_ref.py pins that reference on the CPU and
states the tie figures used here: what retainBest keeps, and the every-tie bound above it.)

1. the synthetic stereo pair at the reference literals (nfeatures 2000) through vsf_extract, vsf_extract_pair and
   vsf_extract_batch_dev: 2039 keypoints for the left image, more than nfeatures;
2. 160x120, (1.2, 8 levels, 300) at edge_threshold 22 and 31, batches of 1, 3 and 9 images of mixed content: a batch that is
   no multiple of 8 (the XCD mapping), levels with 0, 1, 3 and 5 keypoints (KPW - 1 and KPW + 1 of the describe kernel's four);
3. dense_texture (24 096 candidates on level 0: the stage-1 array is HBM-resident in every form) and plateaus (12 877);
4. levels with at most n_l candidates, where raster order stays: line_art at nfeatures 10000, a flat image, one corner;
5. ties: checkerboard(8) fits max_keypoints = nfeatures + 1024, overflows a default context (VSF_ERR_CAPACITY, the truncation
   the HARRIS path documents, and the next call exact again); line_art at (1.2, 8, 500) fits a default context;
6. three pipelined batched calls with an input event over two alternating batches;
7. the selection's production forms at n_points = n_l on the adversarial keys of tests/select_cases.py;
8. a HARRIS context and a FAST_SCORE context in one process, called alternately."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import adversarial_images as adv  # noqa: E402
import orb_score_ref as ref  # noqa: E402
import select_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POISON = 0xA5
FAST_SCORE = 1
SMALL = dict(scale_factor=1.2, nlevels=8)


@pytest.fixture(scope="module")
def capi():
    from vision_slam_frontend_amd import capi
    capi.lib()
    return capi


def _params(capi, w, h, n_images, nfeatures, **over):
    return capi.default_params(w, h, max_images=n_images, nfeatures=nfeatures, score_type=FAST_SCORE, **over)


def _ref_kw(nfeatures, over):
    return dict(nfeatures=nfeatures, **{k: v for k, v in over.items() if k in ("scale_factor", "nlevels", "edge_threshold", "fast_threshold")})


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _dots(w, h, pts, bg=30, fg=220):
    img = np.full((h, w), bg, np.uint8)
    for x, y in pts:
        img[y, x] = fg
    return img


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


def _same(kp, desc, want, what):
    rk, rd = want[0], want[1]
    assert len(kp) == len(rk), "%s: %d keypoints, reference %d" % (what, len(kp), len(rk))
    got = np.ascontiguousarray(kp).view(np.uint8).reshape(-1, 28)
    exp = np.ascontiguousarray(rk).view(np.uint8).reshape(-1, 28)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert len(bad) == 0, "%s: keypoint %d of %d differs: %s, reference %s" % (what, bad[0], len(rk), kp[bad[0]], rk[bad[0]])
    bad = np.nonzero((np.asarray(desc) != rd).any(axis=1))[0]
    assert len(bad) == 0, "%s: descriptor %d of %d differs (keypoint %s)" % (what, bad[0], len(rk), rk[bad[0]])


def _check_batch(kp, de, cn, wants, what, capi):
    kph, deh, cnh = kp.cpu().numpy(), de.cpu().numpy(), cn.cpu().numpy()
    for i, want in enumerate(wants):
        m = len(want[0])
        assert int(cnh[i]) == m, "%s: image %d has %d keypoints, reference %d" % (what, i, int(cnh[i]), m)
        _same(kph[i, :m].reshape(-1).view(capi.KEYPOINT_DTYPE), deh[i, :m], want, "%s image %d" % (what, i))
        assert (kph[i, m:] == POISON).all() and (deh[i, m:] == POISON).all(), "%s: image %d written behind row %d" % (what, i, m)
    n = len(wants)
    assert (kph[n:] == POISON).all() and (deh[n:] == POISON).all() and (cnh[n:] == -1).all(), "%s: written behind the batch" % what


def _batch(ctx, capi, imgs, w, h, n_out=None):
    dev = torch.device("cuda", 0)
    padded, pitch = _packed(imgs, w, h)
    d = torch.from_numpy(padded).to(dev)
    out = _outputs(n_out or len(imgs), ctx.params.max_keypoints, dev)
    ctx.extract_batch_dev(d.data_ptr(), len(imgs), pitch * h, pitch, *[t.data_ptr() for t in out])
    return out


def _check_levels(ctx, image, img, kw, what):
    """vsf_debug_level_keypoints: the list after the one cut, in level coordinates, with its angle."""
    orb = ref.run_oracle(img, **kw)
    for level in range(orb.nlevels):
        want = ref.ic_angles(orb.level_image(level), ref.cut(orb, level))
        got = ctx.debug_level_keypoints(image, level, cap=len(want) + 64)
        assert len(got) == len(want), "%s level %d: %d keypoints, reference %d" % (what, level, len(got), len(want))
        for f in ("x", "y", "size", "angle", "response", "octave"):
            assert np.array_equal(np.ascontiguousarray(got[f]).view(np.uint32), np.ascontiguousarray(want[f]).view(np.uint32)), (what, level, f)


# ---- 1 ----------------------------------------------------------------------------------------------------------------

def test_synthetic_pair_through_every_extract_call(capi, stereo640):
    left, right = stereo640
    wants = [ref.reference(img, 2000) for img in (left, right)]
    assert len(wants[0][0]) == 2039 > 2000  # (counting every tie of every cut: 2057)
    assert set(np.unique(wants[0][0]["response"])) <= set(np.arange(256, dtype=np.float32))  # the FAST score, not Harris
    with capi.Context(_params(capi, 640, 480, 2, 2000)) as ctx:
        assert ctx.params.score_type == FAST_SCORE and ctx.params.max_keypoints == 2256
        for img, want, name in ((left, wants[0], "left"), (right, wants[1], "right")):
            kp, desc = ctx.extract(img)
            _same(kp, desc, want, "vsf_extract " + name)
        _check_levels(ctx, 0, right, dict(nfeatures=2000), "vsf_extract right")
        (k0, d0), (k1, d1) = ctx.extract_pair(left, right)
        _same(k0, d0, wants[0], "vsf_extract_pair left")
        _same(k1, d1, wants[1], "vsf_extract_pair right")
        kp, de, cn = _batch(ctx, capi, [right, left], 640, 480)
        assert ctx.sync() == capi.VSF_OK
        _check_batch(kp, de, cn, [wants[1], wants[0]], "vsf_extract_batch_dev", capi)


# ---- 2 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("border", [22, 31])
def test_small_pyramid_in_batches_of_1_3_9(capi, border):
    from vision_slam_frontend_amd import synth
    w, h = 160, 120
    P = [(40, 40), (80, 60), (120, 45), (60, 80), (100, 80)]
    uniq = [synth.stereo_pair(w, h, 0)[0], _noise(w, h, 1), _dots(w, h, P[:1]), _dots(w, h, P[:3]), _dots(w, h, P[:5]),
            np.full((h, w), 90, np.uint8), synth.stereo_pair(w, h, 3, n_objects=120)[1]]
    over = dict(edge_threshold=border, **SMALL)
    wants = [ref.reference(u, 300, edge_threshold=border, **SMALL) for u in uniq]
    level_counts = {c for want in wants for c in want[2]}
    print("border %d: keypoints per image %s, level counts %s" % (border, [len(x[0]) for x in wants], sorted(level_counts)))
    assert {0, 1, 3, 5} <= level_counts and max(level_counts) > 40  # waves of four that span such levels
    with capi.Context(_params(capi, w, h, 9, 300, **over)) as ctx:
        for n in (1, 3, 9):
            order = [(2 * i + n) % len(uniq) for i in range(n)]
            kp, de, cn = _batch(ctx, capi, [uniq[j] for j in order], w, h, n_out=9)
            assert ctx.sync() == capi.VSF_OK
            _check_batch(kp, de, cn, [wants[j] for j in order], "border %d, %d images" % (border, n), capi)
        _check_levels(ctx, 8, uniq[order[8]], _ref_kw(300, over), "border %d image 8" % border)


# ---- 3 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,level0", [("dense_texture", 24096), ("plateaus", 12877)])
def test_wide_levels(capi, name, level0):
    img = getattr(adv, name)()
    orb = ref.run_oracle(img, nfeatures=2000)
    assert len(orb.stage(0, 0)) == level0 > 12288  # above the largest LDS array of any form: stage 1 starts in HBM
    want = ref.reference(img, 2000)
    with capi.Context(_params(capi, 640, 480, 17, 2000)) as ctx:
        kp, desc = ctx.extract(img)  # a lone frame: the 1024-thread form
        _same(kp, desc, want, name + " vsf_extract")
        flat = np.full((480, 640), 17, np.uint8)
        imgs = [img if i % 4 == 0 else flat for i in range(17)]  # a batch: the 256-thread forms
        out = _batch(ctx, capi, imgs, 640, 480)
        assert ctx.sync() == capi.VSF_OK
        empty = (np.zeros(0, capi.KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8))
        _check_batch(*out, [want if i % 4 == 0 else empty for i in range(17)], name + " batch of 17", capi)


# ---- 4 ----------------------------------------------------------------------------------------------------------------

def test_levels_within_their_budget_keep_raster_order(capi):
    line = adv.line_art()
    orb = ref.run_oracle(line, nfeatures=10000)
    want = ref.reference(line, 10000)
    assert len(want[0]) == 7300
    # level 0 (210 candidates against n_l = 448) and levels 20 .. 37 stay within their budget: the reference keeps raster order there
    within, first = [], 0
    for level in range(orb.nlevels):
        s0 = orb.stage(0, level)
        if 0 < len(s0) <= orb.level_info(level)[3]:
            within.append(level)
            assert want[2][level] == len(s0)
            assert np.array_equal(want[0]["response"][first:first + len(s0)], s0["response"])
        first += want[2][level]
    assert within[0] == 0 and len(within) >= 15, within
    dot = _dots(640, 480, [(320, 240)])
    want_dot = ref.reference(dot, 10000)
    assert want_dot[2][0] == 1 and len(want_dot[0]) == 10 and max(want_dot[2]) == 1  # one corner, seen on ten levels
    flat = np.full((480, 640), 128, np.uint8)
    with capi.Context(_params(capi, 640, 480, 3, 10000)) as ctx:
        _same(*ctx.extract(line), want, "line_art")
        _same(*ctx.extract(dot), want_dot, "one corner")
        K = ctx.params.max_keypoints
        kp = np.full(K, POISON, np.uint8).repeat(28).view(capi.KEYPOINT_DTYPE)
        desc = np.full((K, 32), POISON, np.uint8)
        n = C.c_int(-1)
        st = capi.lib().vsf_extract(ctx._h, flat.ctypes.data_as(C.c_void_p), 640, 480, 640, kp.ctypes.data_as(C.c_void_p),
                                    desc.ctypes.data_as(C.c_void_p), K, C.byref(n))
        assert st == capi.VSF_OK and n.value == 0
        assert (kp.view(np.uint8) == POISON).all() and (desc == POISON).all()
        out = _batch(ctx, capi, [dot, flat, line], 640, 480)
        assert ctx.sync() == capi.VSF_OK
        empty = (np.zeros(0, capi.KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8))
        _check_batch(*out, [want_dot, empty, want], "one corner | flat | line_art", capi)


# ---- 5 ----------------------------------------------------------------------------------------------------------------

def _truncated(capi, img, nfeatures, params, **kw):
    """What an overflowing call leaves: every level cut at its room, the image at max_keypoints; and the count reported."""
    room, _, _ = capi.level_room(params)
    orb = ref.run_oracle(img, nfeatures=nfeatures, **kw)
    lists = [ref.cut(orb, level)[:room[level]] for level in range(orb.nlevels)]
    kp, desc, counts = ref.finish(orb, lists)
    return kp, desc, counts


def test_ties_checkerboard_with_bought_room(capi, stereo640):
    board = adv.checkerboard(8)
    want = ref.reference(board, 2000)
    assert len(want[0]) == 2388 and want[2][2] == 83 + 439  # (every tie: 2698; tests/test_orb_score_ref.py)
    p = _params(capi, 640, 480, 2, 2000, max_keypoints=2000 + 1024)
    assert capi.level_room(p)[0][2] == 83 + 1024
    with capi.Context(p) as ctx:
        _same(*ctx.extract(board), want, "checkerboard(8), max_keypoints = nfeatures + 1024")
        out = _batch(ctx, capi, [board, stereo640[0]], 640, 480)
        assert ctx.sync() == capi.VSF_OK
        _check_batch(*out, [want, ref.reference(stereo640[0], 2000)], "checkerboard | synthetic", capi)


def test_ties_checkerboard_overflows_a_default_context(capi, stereo640):
    board = adv.checkerboard(8)
    p = _params(capi, 640, 480, 2, 2000)
    kp_t, desc_t, counts_t = _truncated(capi, board, 2000, p)
    full = ref.reference(board, 2000)
    # level 2 keeps 522 and holds 83 + 256: the level overflows; what is left (2205) fits the image's 2256
    assert full[2][2] == 522 and counts_t[2] == 339 and sum(counts_t) == 2388 - (522 - 339) == 2205 <= 2256
    with capi.Context(p) as ctx:
        K = ctx.params.max_keypoints
        assert K == 2256
        with pytest.raises(capi.VsfError) as e:
            ctx.extract(board)
        assert e.value.status == capi.VSF_ERR_CAPACITY
        kp = np.zeros(K, capi.KEYPOINT_DTYPE)
        desc = np.zeros((K, 32), np.uint8)
        n = C.c_int()
        st = capi.lib().vsf_extract(ctx._h, board.ctypes.data_as(C.c_void_p), 640, 480, 640, kp.ctypes.data_as(C.c_void_p),
                                    desc.ctypes.data_as(C.c_void_p), K, C.byref(n))
        # as on the HARRIS path: the status, the count of what was kept, every record of it exact (level 2: its first 339)
        assert st == capi.VSF_ERR_CAPACITY and n.value == 2205
        _same(kp[:2205], desc[:2205], (kp_t, desc_t), "checkerboard(8) on a default context")
        # the next call on the same context is exact again, and VSF_OK
        (k0, d0), (k1, d1) = ctx.extract_pair(*stereo640)
        _same(k0, d0, ref.reference(stereo640[0], 2000), "left after the overflow")
        _same(k1, d1, ref.reference(stereo640[1], 2000), "right after the overflow")
        # batched: the status comes with vsf_sync, the neighbour image is exact
        out = _batch(ctx, capi, [stereo640[0], board], 640, 480)
        assert ctx.sync(allow_capacity=True) == capi.VSF_ERR_CAPACITY
        _check_batch(*out, [ref.reference(stereo640[0], 2000), (kp_t, desc_t)], "synthetic | checkerboard", capi)
        assert ctx.sync() == capi.VSF_OK


def test_ties_without_headroom(capi, stereo640):
    """max_keypoints = nfeatures buys no room at all: every level holds its n_l, the synthetic image keeps 2039."""
    img = stereo640[0]
    p = _params(capi, 640, 480, 1, 2000, max_keypoints=2000)
    kp_t, desc_t, counts_t = _truncated(capi, img, 2000, p)
    assert sum(counts_t) == 2000 < 2039
    with capi.Context(p) as ctx:
        kp = np.zeros(2000, capi.KEYPOINT_DTYPE)
        desc = np.zeros((2000, 32), np.uint8)
        n = C.c_int()
        st = capi.lib().vsf_extract(ctx._h, img.ctypes.data_as(C.c_void_p), 640, 480, 640, kp.ctypes.data_as(C.c_void_p),
                                    desc.ctypes.data_as(C.c_void_p), 2000, C.byref(n))
        assert st == capi.VSF_ERR_CAPACITY and n.value == 2000
        _same(kp, desc, (kp_t, desc_t), "synthetic image, max_keypoints = nfeatures")


def test_ties_line_art_fits_a_default_context(capi):
    line = adv.line_art()
    want = ref.reference(line, 500, **SMALL)
    assert len(want[0]) == 583 <= 756 and want[2][0] == 109 + 64  # (every tie: 617)
    with capi.Context(_params(capi, 640, 480, 1, 500, **SMALL)) as ctx:
        assert ctx.params.max_keypoints == 756
        _same(*ctx.extract(line), want, "line_art at (1.2, 8, 500)")


# ---- 6 ----------------------------------------------------------------------------------------------------------------

def test_pipelined_calls_with_an_input_event(capi):
    from vision_slam_frontend_amd import synth
    w, h, N = 352, 160, 32
    dev = torch.device("cuda", 0)
    uniq = [synth.stereo_pair(w, h, f, n_objects=180)[f & 1] for f in range(4)] + [_noise(w, h, 2), adv.checkerboard(8, w, h)]
    wants = [ref.reference(u, 500) for u in uniq]
    orders = [[(i + c) % len(uniq) for i in range(N)] for c in range(2)]
    p = _params(capi, w, h, N, 500, max_keypoints=500 + 1024)

    def run(pipelined):
        with capi.Context(p) as ctx:
            K = ctx.params.max_keypoints
            staged, d_img = [], []
            for order in orders:
                padded, pitch = _packed([uniq[j] for j in order], w, h)
                staged.append(torch.from_numpy(padded).pin_memory())
                d_img.append(torch.zeros(padded.shape, dtype=torch.uint8, device=dev))
            outs = [_outputs(N, K, dev) for _ in range(3)]
            producer = torch.cuda.Stream(device=dev)
            ready = [torch.cuda.Event() for _ in range(3)]
            if pipelined:
                ctx.set_pipeline(True)
                ctx.set_option(capi.OPT_FAST_EARLY_LEVELS, 2)
            for c in range(3):
                b = c & 1
                if pipelined:  # the images arrive late on another stream; the call learns of them through the event alone
                    if c == 2:
                        ctx.sync()  # (buffer 0 is written again: call 0 has read it by now)
                        d_img[b].zero_()
                        torch.cuda.synchronize()
                    with torch.cuda.stream(producer):
                        d_img[b].copy_(staged[b], non_blocking=True)
                        ready[c].record(producer)
                    ctx.set_input_event(ready[c].cuda_event)
                else:
                    d_img[b].copy_(staged[b])
                    torch.cuda.synchronize()
                ctx.extract_batch_dev(d_img[b].data_ptr(), N, pitch * h, pitch, *[t.data_ptr() for t in outs[c]])
            assert ctx.sync() == capi.VSF_OK
            torch.cuda.synchronize()
            return [[t.cpu().numpy() for t in o] for o in outs], outs

    plain, _ = run(False)
    piped, outs = run(True)
    for c in range(3):
        for a, b in zip(plain[c], piped[c]):
            assert np.array_equal(a, b), "pipelined call %d differs from the unpipelined one" % c
        _check_batch(*[torch.from_numpy(x) for x in piped[c]], [wants[j] for j in orders[c & 1]], "pipelined call %d" % c, capi)


# ---- 7 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", "ABCD")
def test_selection_forms_at_the_final_cut(capi, oracle, form):
    """Stage 1 of every production form with n_points = n_l: the budgets of real levels (46 and 90 at nfeatures 2000, 109 at
    (1.2, 8, 500), 414 at 10000) and the positions the adversarial keys were made for -- in this mode any of them can be a
    level's n_l, and what the depth-limit fallback leaves is the output order."""
    fallbacks = checked = 0
    with capi.Context(capi.default_params(320, 240, max_images=1, nfeatures=100, score_type=FAST_SCORE)) as ctx:
        for c in sc.killer_cases(form, oracle) + sc.mod256_cases(oracle):
            if c.stage != 1:
                continue
            for k in sorted(set(c.n_points) | {n_l for n_l in (46, 90, 109, 414) if n_l < len(c.keys)}):
                p = sc.path_of(form, 1, c.keys, k, oracle)
                fallbacks += p is not None and p.regime is not None
                rk, rid = oracle.retain_best(c.keys, k)
                gk, gid, intact = ctx.debug_retain_best_form(form, 1, c.keys, k)
                what = "form %s %s n=%d n_points=%d" % (form, c.name, len(c.keys), k)
                assert len(gid) == len(rid), what
                np.testing.assert_array_equal(gid, rid, err_msg=what)
                np.testing.assert_array_equal(gk, rk.astype(np.uint32), err_msg=what)
                assert intact, what
                checked += 1
    print("form %s: %d selections, %d through the depth-limit fallback" % (form, checked, fallbacks))
    assert fallbacks >= 20 and checked >= 60


# ---- 8 ----------------------------------------------------------------------------------------------------------------

def test_harris_context_beside_a_fast_score_context(capi, oracle, stereo640):
    left, right = stereo640
    board = adv.checkerboard(8)
    harris = {}
    for name, img in (("left", left), ("right", right), ("board", board)):
        o = oracle.Orb(nfeatures=2000)
        o.run(img)
        harris[name] = o.result()
    fast = {"left": ref.reference(left, 2000), "right": ref.reference(right, 2000), "board": ref.reference(board, 2000)}
    assert harris["left"][0].tobytes() != fast["left"][0][:len(harris["left"][0])].tobytes()
    with capi.Context(capi.default_params(640, 480, max_images=2, nfeatures=2000)) as hc, \
            capi.Context(_params(capi, 640, 480, 2, 2000, max_keypoints=3024)) as fc:
        assert (hc.params.score_type, fc.params.score_type) == (0, 1)
        for name, img in (("left", left), ("board", board), ("right", right)):
            _same(*fc.extract(img), fast[name], "FAST_SCORE " + name)
            _same(*hc.extract(img), harris[name], "HARRIS " + name)
        # ... and with both contexts' batched calls in flight at once
        dev = torch.device("cuda", 0)
        padded, pitch = _packed([left, board], 640, 480)
        d = torch.from_numpy(padded).to(dev)
        ho, fo = _outputs(2, hc.params.max_keypoints, dev), _outputs(2, fc.params.max_keypoints, dev)
        for _ in range(2):
            hc.extract_batch_dev(d.data_ptr(), 2, pitch * 480, pitch, *[t.data_ptr() for t in ho])
            fc.extract_batch_dev(d.data_ptr(), 2, pitch * 480, pitch, *[t.data_ptr() for t in fo])
        assert hc.sync() == capi.VSF_OK and fc.sync() == capi.VSF_OK
        _check_batch(*ho, [harris["left"], harris["board"]], "HARRIS batch", capi)
        _check_batch(*fo, [fast["left"], fast["board"]], "FAST_SCORE batch", capi)
