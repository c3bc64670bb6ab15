"""Reference for cv::ORB::FAST_SCORE (vsf_params::score_type 1), built on the unmodified CPU oracle.

OpenCV 3.2 computeKeyPoints with scoreType == FAST_SCORE runs, per level, FAST + runByImageBorder and ONE
retainBest(n_l) on the FAST score; HarrisResponses and the second cut are skipped.  Everything behind that is what the
HARRIS path does.  The oracle runs HARRIS mode only, but it exposes all this mode consumes:

  step 1  the oracle itself, same remaining parameters: the stage-0 list of every level (raster order, after
          runByImageBorder), n_l, the scale, the unblurred and the blurred level image;
  step 2  the cut: oracle.retain_best(score, n_l) -- the host libstdc++ permutation: std::nth_element, then every
          candidate behind position n_l whose score is not below that of element n_l - 1 (one of the best n_l as
          nth_element left them, not always the lowest: part of the cut's ties can fall away, tie_row counts both ways);
  step 3  ICAngles on the unblurred level: integer moments over the umax disc, then the oracle's fast_atan2;
  step 4  computeOrbDescriptors (WTA_K 2) on the blurred level with the oracle's rounding rules (oracle/vsf_oracle.cc,
          OrbDescriptor): cos / sin as the correctly rounded float of the float angle, float products without
          contraction, cvRound (half to even) of the rotated pattern.  Every read lies inside the level because
          edge_threshold >= 22.

Steps 3 and 4 are restated here; tests/test_orb_score_ref.py pins them by feeding the oracle's OWN stage-3 lists through
them, which must reproduce vsfo_orb_result bit for bit.  After that the reference differs from the oracle in one thing:
which list goes in."""
from __future__ import annotations

import numpy as np

from oracle import binding as ob

HALF = 15  # patch_size 31
# the end of each row of the circular patch (computeKeyPoints' umax for patch_size 31)
UMAX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)


def _disc():
    v, u = np.mgrid[-HALF:HALF + 1, -HALF:HALF + 1]
    inside = np.abs(u) <= np.array(UMAX)[np.abs(v)]
    return u[inside].astype(np.int64), v[inside].astype(np.int64)


_DISC_U, _DISC_V = _disc()


def run_oracle(img, nfeatures, scale_factor=1.04, nlevels=50, edge_threshold=31, fast_threshold=20):
    """Step 1.  Returns the oracle object after its (HARRIS) run; its stages and level images are what the steps below read."""
    orb = ob.Orb(nfeatures=nfeatures, scale_factor=scale_factor, nlevels=nlevels, edge_threshold=edge_threshold,
                 fast_threshold=fast_threshold)
    orb.run(img)
    return orb


def cut(orb, level):
    """Step 2: the level's list after retainBest(n_l) on the FAST score, with octave and size set as computeKeyPoints does."""
    _, _, scale, n_l = orb.level_info(level)
    s0 = orb.stage(0, level)
    _, ids = ob.retain_best(s0["response"], n_l)
    kp = s0[ids].copy()
    kp["octave"] = level
    kp["size"] = np.float32(31) * np.float32(scale)
    return kp


def ic_angles(level_img, kp):
    """Step 3: kp["angle"] from the integer moments of the unblurred level (level coordinates)."""
    out = kp.copy()
    if len(kp) == 0:
        return out
    x = np.rint(kp["x"]).astype(np.int64)
    y = np.rint(kp["y"]).astype(np.int64)
    px = level_img[(y[:, None] + _DISC_V[None, :]), (x[:, None] + _DISC_U[None, :])].astype(np.int64)
    m10 = (px * _DISC_U[None, :]).sum(axis=1)
    m01 = (px * _DISC_V[None, :]).sum(axis=1)
    out["angle"] = [ob.fast_atan2(float(np.float32(a)), float(np.float32(b))) for a, b in zip(m01, m10)]
    return out


def descriptors(blurred, scale, kp0):
    """Step 4: the 32-byte descriptors of kp0 (LEVEL-0 coordinates, angle set) on the blurred level of that scale."""
    n = len(kp0)
    if n == 0:
        return np.zeros((0, 32), np.uint8)
    f32 = np.float32
    pat = ob.orb_pattern31().reshape(-1, 2).astype(f32)  # 512 points (x, y)
    inv = f32(1.0) / f32(scale)
    angle = kp0["angle"].astype(f32) * f32(np.pi / float(f32(180.0)))
    a = np.cos(angle.astype(np.float64)).astype(f32)[:, None]
    b = np.sin(angle.astype(np.float64)).astype(f32)[:, None]
    cx = np.rint(kp0["x"].astype(f32) * inv).astype(np.int64)[:, None]
    cy = np.rint(kp0["y"].astype(f32) * inv).astype(np.int64)[:, None]
    ppx, ppy = pat[None, :, 0], pat[None, :, 1]
    rx = (ppx * a).astype(f32) - (ppy * b).astype(f32)
    ry = (ppx * b).astype(f32) + (ppy * a).astype(f32)
    ix = np.rint(rx.astype(f32)).astype(np.int64)
    iy = np.rint(ry.astype(f32)).astype(np.int64)
    val = blurred[cy + iy, cx + ix].astype(np.int32)  # [n][512]
    bits = (val[:, 0::2] < val[:, 1::2]).astype(np.uint8).reshape(n, 32, 8)
    return (bits << np.arange(8, dtype=np.uint8)[None, None, :]).sum(axis=2).astype(np.uint8)


def finish(orb, lists):
    """Steps 3 and 4 on per-level lists (level coordinates, octave and size set): (keypoints, descriptors, counts per level)
    in output order -- level-major, the list's own order inside a level; pt *= scale."""
    kps, descs, counts = [], [], []
    for level, kp in enumerate(lists):
        _, _, scale, _ = orb.level_info(level)
        counts.append(len(kp))
        if len(kp) == 0:
            continue
        k = ic_angles(orb.level_image(level), kp)
        k["x"] = k["x"] * np.float32(scale)
        k["y"] = k["y"] * np.float32(scale)
        kps.append(k)
        descs.append(descriptors(orb.level_image(level, blurred=True), scale, k))
    if not kps:
        return np.zeros(0, ob.KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), counts
    return np.concatenate(kps), np.concatenate(descs), counts


def level_lists(orb):
    return [cut(orb, level) for level in range(orb.nlevels)]


def tie_row(orb, every_tie=False):
    """(total kept, worst level excess kept - n_l, (that level, its n_l, its candidates), levels that keep more than
    2 n_l + 64) from the stage-0 lists alone.  every_tie: count every candidate whose score is not below the n_l-th best
    score -- the most ANY permutation std::nth_element may leave lets retainBest keep -- instead of what the oracle's
    retainBest keeps (its threshold is element n_l - 1 behind nth_element: one of the best n_l, not always the lowest)."""
    total, worst, wide = 0, (0, (0, 0, 0)), 0
    for level in range(orb.nlevels):
        _, _, _, n_l = orb.level_info(level)
        score = orb.stage(0, level)["response"]
        if every_tie:
            kept = len(score) if len(score) <= n_l else 0 if n_l == 0 else int((score >= np.sort(score)[::-1][n_l - 1]).sum())
        else:
            kept = len(ob.retain_best(score, n_l)[1])
        total += kept
        wide += kept > 2 * n_l + 64
        if kept - n_l > worst[0]:
            worst = (kept - n_l, (level, n_l, len(score)))
    return total, worst[0], worst[1], wide


_cache = {}


def reference(img, nfeatures, scale_factor=1.04, nlevels=50, edge_threshold=31, fast_threshold=20):
    """detectAndCompute in FAST_SCORE mode: (keypoints, descriptors, counts per level).  Computed once per input and kept
    (the returned arrays are shared: leave them unchanged)."""
    key = (img.tobytes(), img.shape, nfeatures, float(np.float32(scale_factor)), nlevels, edge_threshold, fast_threshold)
    if key not in _cache:
        orb = run_oracle(img, nfeatures, scale_factor, nlevels, edge_threshold, fast_threshold)
        _cache[key] = finish(orb, level_lists(orb))
    return _cache[key]
