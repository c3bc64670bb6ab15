"""Reference for cv::ORB::detectAndCompute(image, mask, ...) built on the unmodified CPU oracle (which runs without a mask).

OpenCV 3.2, restated from memory (orb.cpp / keypoint.cpp; include/vsf.h "Detection masks" states the same rule):

  step 1  the oracle on the image, unmasked: the stage-0 list of every level (raster order, after runByImageBorder), n_l, the
          scale, the unblurred and the blurred level image;
  step 2  the mask pyramid: level 0 is the mask, level l is tozero254(oracle.resize_linear(level l - 1, size_l)) -- built from
          the already thresholded level below, never from level 0;
  step 3  KeyPointsFilter::runByPixelsMask: keep the stage-0 entries whose own pixel is non-zero in their level's mask (the
          filter runs before runByImageBorder in OpenCV; the two are predicates on one raster-order list and commute);
  step 4  HARRIS_SCORE: oracle.retain_best(FAST score, 2 n_l), HarrisResponses restated in numpy (7 x 7 block, k = 0.04, the
          oracle's float order), oracle.retain_best(harris, n_l); FAST_SCORE: oracle.retain_best(score, n_l);
  step 5  orb_score_ref's ic_angles, descriptors and finish (pinned there against the oracle).

tests/test_orb_mask_ref.py pins the restated parts: with step 3 skipped (or an all-255 mask) the reference reproduces
vsfo_orb_result bit for bit."""
from __future__ import annotations

import numpy as np

import orb_score_ref as sref
from oracle import binding as ob

HARRIS, FAST_SCORE = 0, 1


def tozero254(img):
    """threshold(img, 254, 0, THRESH_TOZERO): values above 254 stay, the rest become 0."""
    return np.where(img > 254, img, 0).astype(np.uint8)


def mask_pyramid(mask, sizes):
    """Step 2.  sizes: (w, h) of every level; level 0 is `mask` itself (its values, not 0 / 255)."""
    levels = [np.ascontiguousarray(mask, np.uint8)]
    for w, h in sizes[1:]:
        levels.append(tozero254(ob.resize_linear(levels[-1], w, h)))
    return levels


def level_sizes(orb):
    return [orb.level_info(level)[:2] for level in range(orb.nlevels)]


def filter_by_mask(kp, mask_level):
    """Step 3 on one level's list (level coordinates, integers as FAST leaves them)."""
    if len(kp) == 0:
        return kp
    x = (kp["x"] + np.float32(0.5)).astype(np.int64)
    y = (kp["y"] + np.float32(0.5)).astype(np.int64)
    return kp[mask_level[y, x] != 0]


def harris_responses(level_img, kp):
    """HarrisResponses(blockSize 7, k 0.04) in the oracle's float order: kp with its response replaced."""
    out = kp.copy()
    if len(kp) == 0:
        return out
    f32 = np.float32
    img = level_img.astype(np.int64)
    x0 = np.rint(kp["x"]).astype(np.int64)
    y0 = np.rint(kp["y"]).astype(np.int64)
    dy, dx = np.mgrid[-3:4, -3:4]
    yy = y0[:, None] + dy.reshape(-1)[None, :]
    xx = x0[:, None] + dx.reshape(-1)[None, :]

    def px(oy, ox):
        return img[yy + oy, xx + ox]

    ix = (px(0, 1) - px(0, -1)) * 2 + (px(-1, 1) - px(-1, -1)) + (px(1, 1) - px(1, -1))
    iy = (px(1, 0) - px(-1, 0)) * 2 + (px(1, -1) - px(-1, -1)) + (px(1, 1) - px(-1, 1))
    a = (ix * ix).sum(axis=1)
    b = (iy * iy).sum(axis=1)
    c = (ix * iy).sum(axis=1)
    assert max(a.max(), b.max(), np.abs(c).max()) < 2 ** 31  # (the oracle sums in int)
    scale = f32(1.0) / (f32(4 * 7) * f32(255.0))
    scale4 = scale * scale * scale * scale
    af, bf, cf = a.astype(f32), b.astype(f32), c.astype(f32)
    s = af + bf
    out["response"] = (af * bf - cf * cf - f32(0.04) * s * s) * scale4
    return out


def level_list(orb, level, mask_level, score_type):
    """Steps 3 and 4 of one level: the list behind the cuts, octave and size set as computeKeyPoints does."""
    _, _, scale, n_l = orb.level_info(level)
    kp = orb.stage(0, level)
    if mask_level is not None:
        kp = filter_by_mask(kp, mask_level)
    if score_type == FAST_SCORE:
        _, ids = ob.retain_best(kp["response"], n_l)
        kp = kp[ids].copy()
    else:
        _, ids = ob.retain_best(kp["response"], 2 * n_l)
        kp = harris_responses(orb.level_image(level), kp[ids])
        _, ids = ob.retain_best(kp["response"], n_l)
        kp = kp[ids].copy()
    kp["octave"] = level
    kp["size"] = np.float32(31) * np.float32(scale)
    return kp


_cache = {}
_orbs = {}


def run_oracle(img, nfeatures, **kw):
    """Step 1, once per (image, parameters): shared among masks and modes."""
    key = (img.tobytes(), img.shape, nfeatures, tuple(sorted(kw.items())))
    if key not in _orbs:
        _orbs[key] = sref.run_oracle(img, nfeatures, **kw)
    return _orbs[key]


def reference(img, mask, nfeatures, score_type=HARRIS, skip_filter=False, **kw):
    """detectAndCompute(img, mask): (keypoints, descriptors, counts per level).  mask None: no mask.  Computed once per input
    and kept (the returned arrays are shared: leave them unchanged).  skip_filter: step 3 left out (the pin)."""
    orb = run_oracle(img, nfeatures, **kw)
    key = (img.tobytes(), img.shape, None if mask is None else mask.tobytes(), nfeatures, score_type, skip_filter,
           tuple(sorted(kw.items())))
    if key not in _cache:
        pyr = None if (mask is None or skip_filter) else mask_pyramid(mask, level_sizes(orb))
        lists = [level_list(orb, level, None if pyr is None else pyr[level], score_type) for level in range(orb.nlevels)]
        _cache[key] = sref.finish(orb, lists)
    return _cache[key]


# ---- the masks the tests use, at any size ----------------------------------------------------------------------------------

def masks(w, h):
    """name -> (h, w) uint8 mask: the cases of tests/test_gpu_mask.py's pyramid test."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = {
        "all255": np.full((h, w), 255, np.uint8),
        "all0": np.zeros((h, w), np.uint8),
        "all254": np.full((h, w), 254, np.uint8),
        "half_plane": np.where(xx < w // 2 + 3, 255, 0).astype(np.uint8),
        "rectangle_two_borders": np.where((xx >= w - w // 3) & (yy >= h - h // 2), 0, 255).astype(np.uint8),
        "checkerboard2": np.where(((xx // 2) + (yy // 2)) % 2 == 0, 255, 0).astype(np.uint8),
        "holes": np.full((h, w), 255, np.uint8),
        "single_pixels": np.zeros((h, w), np.uint8),
        "stripes_1_128_254_255": np.array([1, 128, 254, 255], np.uint8)[(xx // 5) % 4],
        "disc": np.where((xx - w * 0.55) ** 2 + (yy - h * 0.45) ** 2 < (min(w, h) * 0.38) ** 2, 255, 0).astype(np.uint8),
    }
    rng = np.random.default_rng(7)
    for _ in range(40):
        out["holes"][rng.integers(0, h), rng.integers(0, w)] = 0
        out["single_pixels"][rng.integers(0, h), rng.integers(0, w)] = 255
    return out


# ---- the scenes of the GPU tests (tests/test_orb_mask_ref.py checks on the CPU that each of them exercises the feature) -----

SMALL = dict(scale_factor=1.2, nlevels=8)


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def scenes():
    """name -> (image, mask, nfeatures, oracle keywords)."""
    from vision_slam_frontend_amd import synth
    m160, m97, m640 = masks(160, 120), masks(97, 75), masks(640, 480)
    return {
        "noise160_half": (_noise(160, 120, 1), m160["half_plane"], 300, dict(SMALL)),
        "noise160_disc": (_noise(160, 120, 5), m160["disc"], 300, dict(SMALL)),
        "synth160_rect": (synth.stereo_pair(160, 120, 0, n_objects=150)[0], m160["rectangle_two_borders"], 120, dict(edge_threshold=22, **SMALL)),
        "noise97_stripes": (_noise(97, 75, 2), m97["stripes_1_128_254_255"], 40, dict(edge_threshold=22, **SMALL)),
        "noise97_half": (_noise(97, 75, 3), m97["half_plane"], 40, dict(edge_threshold=22, **SMALL)),
        "synth640_disc": (synth.stereo_pair(640, 480, 0)[0], m640["disc"], 2000, dict()),
    }


def bites(img, mask, nfeatures, score_type, **kw):
    """What a (scene, mask) has to show for a test on it to mean something: (differs, levels with more than 2 n_l candidates
    behind the filter, levels where the masked result holds a corner the unmasked one does not: a freed slot refilled)."""
    orb = run_oracle(img, nfeatures, **kw)
    pyr = mask_pyramid(mask, level_sizes(orb))
    plain = reference(img, None, nfeatures, score_type, **kw)
    masked = reference(img, mask, nfeatures, score_type, **kw)
    differs = plain[0].tobytes() != masked[0].tobytes()
    crowded, refilled = [], []
    p0 = m0 = 0
    for level in range(orb.nlevels):
        n_l = orb.level_info(level)[3]
        if len(filter_by_mask(orb.stage(0, level), pyr[level])) > 2 * n_l:
            crowded.append(level)
        a = plain[0][p0:p0 + plain[2][level]]
        b = masked[0][m0:m0 + masked[2][level]]
        p0 += plain[2][level]
        m0 += masked[2][level]
        if set(zip(b["x"].tolist(), b["y"].tolist())) - set(zip(a["x"].tolist(), a["y"].tolist())):
            refilled.append(level)
    return differs, crowded, refilled
