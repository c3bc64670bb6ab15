"""Cross-checks of the oracle against an INDEPENDENT third-party implementation: scikit-image 0.18.3.  It is neither the
reference nor OpenCV, so this does not pin parity with the reference (DESIGN.md section 2 stays "parity unpinned"); it does
show that three definitions the oracle restates from memory of OpenCV are not misremembered:
  * the FAST-9/16 segment test (the set of corners before non-max suppression),
  * the intensity-centroid orientation over the radius-15 disc (skimage's OFAST_MASK = OpenCV's umax table),
  * rotated BRIEF: pattern table, rotation, sampling, comparison and bit order (skimage ships OpenCV's bit_pattern_31_).
scikit-image's answers (tests/third_party/skimage_probe.py) are stored in tests/golden/skimage/ together with a digest of the
inputs they were computed from (tests/skimage_golden.py; refreshed by tools/make_skimage_golden.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import skimage_golden as skg  # noqa: E402


@pytest.fixture(scope="module")
def image320():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    from vision_slam_frontend_amd import synth
    return synth.stereo_pair(320, 240, 3, n_objects=300)[0]


@pytest.mark.parametrize("threshold", [10, 20, 40])
def test_fast9_corner_set_equals_skimage(oracle, image320, threshold):
    theirs = skg.corner_set("synth320", image320, threshold)
    kp = oracle.fast9_16(image320, threshold, nms=False)
    ours = set(zip(kp["x"].astype(int).tolist(), kp["y"].astype(int).tolist()))
    assert len(ours) > 3000
    assert ours == theirs


def test_ic_angle_agrees_with_skimage(oracle, image320):
    img, pts, kp = skg.angle_input(oracle, image320)
    assert len(kp) > 500
    theirs = np.degrees(skg.angles("synth320", img, pts)) % 360.0
    diff = np.abs(((kp["angle"] - theirs) + 180.0) % 360.0 - 180.0)
    assert diff.max() < 0.3  # cv::fastAtan2's documented accuracy; measured: < 0.01 degrees


def test_rotated_brief_bits_equal_skimage(oracle, image320):
    # one level: final keypoints are level coordinates
    blurred, pts, ang, desc = skg.desc_input(oracle, image320)
    assert len(pts) == len(desc) > 500
    theirs = skg.brief_bits("synth320", blurred, pts, ang)
    ours = np.unpackbits(desc, axis=1, bitorder="little")  # bit i of byte k = pair 8 k + i
    # (float vs double trig may move a sample across a rounding boundary once in a long while: allow a stray bit)
    ham = (theirs != ours).sum(1)
    assert ham.max() <= 2 and (ham == 0).mean() > 0.98
