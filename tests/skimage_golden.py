"""scikit-image's answers for the oracle cross-checks (tests/test_third_party_crosscheck.py, test_real_images.py), stored in
tests/golden/skimage/crosscheck.npz so that the checks need no interpreter with scikit-image.  tests/third_party/
skimage_probe.py computed them (tools/make_skimage_golden.py) from the very inputs the tests build with the oracle; each
answer carries a sha256 of those inputs, and a test first checks that the oracle still produces them.

    <case>__fast<t>      FAST-9 corner set (no NMS) at threshold t, a packed bit mask over the image
    <case>__angle        intensity-centroid orientation (radians) at the oracle's level-0 keypoints
    <case>__desc         256 rotated-BRIEF bits per keypoint, packed little-endian (bit i of byte k = pair 8 k + i)
    <case>__<what>_sha   sha256 of the probe's input arrays"""
import hashlib
from pathlib import Path

import numpy as np

GOLD = Path(__file__).resolve().parent / "golden" / "skimage" / "crosscheck.npz"
CASES = {"synth320": (10, 20, 40), "camera": (20,), "motorcycle_left": (20,), "gravel": (20,)}
_cache = {}


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def load():
    if "g" not in _cache:
        with np.load(GOLD) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def fast_input(img):
    return (img,)


def angle_input(oracle, img):
    """(image, int32 (x, y) of the level-0 keypoints of a one-level ORB with 2000 features, those keypoints)."""
    o = oracle.Orb(nfeatures=2000, nlevels=1)
    o.run(img)
    kp = o.stage(4, 0)
    return img, np.stack([kp["x"].astype(np.int32), kp["y"].astype(np.int32)], 1), kp


def desc_input(oracle, img):
    """(blurred level 0, int32 (x, y), angles in radians, the oracle's descriptors) of the same one-level ORB."""
    o = oracle.Orb(nfeatures=2000, nlevels=1)
    o.run(img)
    _, desc = o.result()
    kp = o.stage(4, 0)
    pts = np.stack([kp["x"].astype(np.int32), kp["y"].astype(np.int32)], 1)
    return o.level_image(0, blurred=True), pts, np.radians(kp["angle"].astype(np.float64)), desc


def _checked(case, what, inputs):
    g = load()
    assert digest(*inputs) == str(g["%s__%s_sha" % (case, what)]), (
        "the oracle's inputs for %s / %s differ from the ones scikit-image's answer was computed from: refresh it with "
        "tools/make_skimage_golden.py" % (case, what))
    return g


def corner_set(case, img, threshold):
    """scikit-image's FAST-9 corners of `img` as a set of (x, y)."""
    g = _checked(case, "fast", fast_input(img))
    mask = np.unpackbits(g["%s__fast%d" % (case, threshold)])[:img.size].reshape(img.shape).astype(bool)
    ys, xs = np.nonzero(mask)
    return set(zip(xs.tolist(), ys.tolist()))


def angles(case, img, pts):
    """scikit-image's orientation (radians) at `pts` on `img`."""
    return _checked(case, "angle", (img, pts))["%s__angle" % case]


def brief_bits(case, blurred, pts, ang):
    """scikit-image's rotated-BRIEF bits, (n, 256) uint8."""
    g = _checked(case, "desc", (blurred, pts, ang))
    return np.unpackbits(g["%s__desc" % case], axis=1, bitorder="little")
