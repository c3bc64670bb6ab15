"""FAST's score network (k_fast.hip, score_from_circle) on the GPU, byte for byte against the CPU oracle.

The network takes the minimum of every four consecutive circle pixels (F) from the four odd pixel pairs (E) and two
three-input ops per pair of quads, one form for even and one for odd quads; the arc terms (T) join two quads and the two
pixels beside them.  The images here put every one of these terms in charge of a decision:

  * arc images: 7x7 tiles on an 8-pixel grid (a tile holds one whole circle, and with FAST's 3-pixel rim every tile centre
    of the image is a valid pixel).  For a threshold t, each of the 16 arc starts, both polarities and the centres t + 20,
    128 and 255 - t - 20 there is a tile whose arc of NINE circle pixels is centre +- (t + 1 + k), k in 0 .. 19 (0 and 19
    in every arc, so circle values reach 0 and 255: the ends of the range the three-input ops see as f16 denormals), all
    other pixels at the centre value -- a corner -- and the same tile with an arc of EIGHT, which is none.  (A tile whose
    values would leave 0 .. 255 does not exist: at t = 200 only the dark arcs on centre 220 and the bright ones on 35.)
    The test first asks the oracle itself that the tiles are what they claim to be;
  * noise in 100 .. 107, where neighbours tie in score all the time (the strict suppression on equal scores), full-range
    noise, and a checkerboard of 0 / 255 in squares of 3 pixels.

Every image runs through the standalone detector (one level, so small images are valid) at thresholds 0, 1, 20 and 200,
with and without NMS, at 96x40 (one packed work item) and 272x80 (a full 248-column cell plus a packed remainder): the
smallest shapes that take both march forms (test_shapes_take_both_march_forms); larger ones are tests/test_gpu_fast_packed.py's.
One whole extraction of the 272x80 arc image (t = 20, ORB's FAST threshold) tiled to 272x160 is compared with oracle.Orb."""
import ctypes as C
import functools

import numpy as np
import pytest

THRESHOLDS = (0, 1, 20, 200)
SIZES = ((96, 40), (272, 80))
# Bresenham circle of radius 3 in OpenCV's order
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
          (-3, 1), (-2, 2), (-1, 3))
K_OF_ARC_PIXEL = (19, 0, 7, 3, 12, 5, 16, 9, 1)  # rotated by the arc's start; always holds 0 and 19
GROUND = 128


@pytest.fixture(scope="module")
def capi():
    from vision_slam_frontend_amd import capi
    capi.lib()
    return capi


@functools.lru_cache(maxsize=None)
def arc_tiles(t):
    """(7x7 tile, is a corner at threshold t) for every arc start, polarity, centre and the arc lengths 9 and 8"""
    tiles = []
    for centre in (t + 20, 128, 255 - t - 20):
        for pol in (1, -1):
            if not 0 <= centre + pol * (t + 20) <= 255:
                continue
            for length in (9, 8):
                for start in range(16):
                    tile = np.full((7, 7), centre, np.int32)
                    for i in range(length):
                        dx, dy = CIRCLE[(start + i) % 16]
                        tile[3 + dy, 3 + dx] = centre + pol * (t + 1 + K_OF_ARC_PIXEL[(i + start) % 9])
                    assert tile.min() >= 0 and tile.max() <= 255
                    tiles.append((tile.astype(np.uint8), length == 9))
    values = np.concatenate([tl.ravel() for tl, _ in tiles])
    assert values.min() == 0 and values.max() == 255
    return tiles


@functools.lru_cache(maxsize=None)
def arc_images(w, h, t):
    """[(image, [(x, y, is a corner)] of its tile centres)]: as many images as it takes to show every tile of arc_tiles(t);
    the slots left in the last one repeat the list from its start"""
    tiles = arc_tiles(t)
    per_image = (w // 8) * (h // 8)
    out = []
    for first in range(0, len(tiles), per_image):
        img, centres = np.full((h, w), GROUND, np.uint8), []
        for slot in range(per_image):
            tile, corner = tiles[(first + slot) % len(tiles)]
            x0, y0 = 8 * (slot % (w // 8)), 8 * (slot // (w // 8))
            img[y0:y0 + 7, x0:x0 + 7] = tile
            centres.append((x0 + 3, y0 + 3, corner))
        img.setflags(write=False)
        out.append((img, centres))
    return out


@functools.lru_cache(maxsize=None)
def noise_images(w, h):
    rng = np.random.default_rng(1000 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    imgs = [rng.integers(100, 108, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8),
            (((xx // 3 + yy // 3) & 1) * 255).astype(np.uint8)]
    for im in imgs:
        im.setflags(write=False)
    return imgs


def same_as_oracle(ctx, oracle, img, nms, what):
    for thr in THRESHOLDS:
        want = oracle.fast9_16(img, thr, nms)
        got = ctx.fast_detect(img, thr, nms, cap=img.size)
        assert len(got) == len(want), (what, thr)
        assert got.tobytes() == want.tobytes(), (what, thr)


def test_shapes_take_both_march_forms(capi):
    """96x40: packed items only; 272x80: full cells and packed items (the decomposition itself: tests/test_fast_packing.py)"""
    for (w, h), want_full in zip(SIZES, (False, True)):
        for nms in (1, 0):
            p = capi.default_params(w, h, max_images=1, nfeatures=100)
            words = np.zeros(1 << 12, np.uint32)
            levels = np.zeros((64, 10), np.int32)
            nw, nf = C.c_int(), C.c_int()
            assert capi.lib().vsf_debug_fast_work(C.byref(p), 0, nms, words.ctypes.data, len(words), C.byref(nw), C.byref(nf),
                                                  levels.ctypes.data, 64) == capi.VSF_OK
            assert (nf.value > 0) == want_full and nw.value > nf.value, (w, h, nf.value, nw.value)


def test_arc_tiles_are_what_they_claim(oracle):
    for w, h in SIZES:
        for t in THRESHOLDS:
            images = arc_images(w, h, t)
            # every arc start of both lengths and polarities; every tile has a slot
            assert len(arc_tiles(t)) >= 2 * 2 * 16 and sum(len(c) for _, c in images) >= len(arc_tiles(t))
            for img, centres in images:
                found = {(int(k["x"]), int(k["y"])) for k in oracle.fast9_16(img, t, False)}
                for x, y, corner in centres:
                    assert ((x, y) in found) == corner, (w, h, t, x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("nms", [True, False])
def test_arc_images(capi, oracle, w, h, nms):
    with capi.Context(capi.default_params(w, h, max_images=1, nfeatures=100)) as ctx:
        for t in THRESHOLDS:
            for k, (img, _) in enumerate(arc_images(w, h, t)):
                same_as_oracle(ctx, oracle, img, nms, "arcs for t=%d, image %d" % (t, k))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("nms", [True, False])
def test_noise_and_checkerboard(capi, oracle, w, h, nms):
    with capi.Context(capi.default_params(w, h, max_images=1, nfeatures=100)) as ctx:
        for name, img in zip(("noise 100..107", "noise 0..255", "checkerboard"), noise_images(w, h)):
            same_as_oracle(ctx, oracle, img, nms, name)


@pytest.mark.gpu
def test_extract_arc_image(capi, oracle):
    """272x160 keeps 210x98 pixels inside ORB's 31-pixel border at level 0 and the oracle finds well over 20 keypoints
    there, so the larger 333x257 is not needed."""
    img = np.ascontiguousarray(np.tile(arc_images(272, 80, 20)[0][0], (2, 1)))
    assert img.shape == (160, 272)
    o = oracle.Orb(nfeatures=500)
    o.run(img)
    rk, rd = o.result()
    assert len(rk) >= 20
    with capi.Context(capi.default_params(272, 160, max_images=1, nfeatures=500)) as ctx:
        kp, desc = ctx.extract(img)
    assert len(kp) == len(rk)
    assert kp.tobytes() == rk.tobytes()
    np.testing.assert_array_equal(desc, rd)
