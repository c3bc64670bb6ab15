#!/usr/bin/env python3
"""Writes tests/golden/skimage/crosscheck.npz: scikit-image's answers (tests/third_party/skimage_probe.py) on the inputs
the oracle cross-checks build (tests/skimage_golden.py), so that those checks run without scikit-image.

    python tools/make_skimage_golden.py PYTHON

PYTHON: an interpreter with scikit-image (the probe was written against 0.18.3).  scikit-image is third-party software,
neither the reference nor OpenCV: these vectors show that three definitions the oracle restates are not misremembered."""
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import skimage_golden as skg  # noqa: E402
from oracle import binding as ob  # noqa: E402
from vision_slam_frontend_amd import synth  # noqa: E402

PROBE = ROOT / "tests" / "third_party" / "skimage_probe.py"


def case_image(case):
    if case == "synth320":
        return synth.stereo_pair(320, 240, 3, n_objects=300)[0]
    from PIL import Image
    return np.asarray(Image.open(ROOT / "tests" / "golden" / "real" / (case + ".png")))


def main(py):
    ob.build()
    ob.lib()
    out = {}
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)

        def probe(mode, *arrays, extra=()):
            paths = []
            for i, a in enumerate(arrays):
                np.save(td / ("in%d.npy" % i), a)
                paths.append(td / ("in%d.npy" % i))
            args = [str(paths[0]), *map(str, extra), *map(str, paths[1:]), str(td / "out.npy")]
            subprocess.check_call([py, str(PROBE), mode, *args], stdout=subprocess.DEVNULL,
                                  env=dict(os.environ, PYTHONWARNINGS="ignore"))
            return np.load(td / "out.npy")

        for case, thresholds in skg.CASES.items():
            img = case_image(case)
            out["%s__fast_sha" % case] = np.array(skg.digest(*skg.fast_input(img)))
            for t in thresholds:
                xy = probe("fast", img, extra=(t,))
                mask = np.zeros(img.shape, bool)
                mask[xy[:, 1], xy[:, 0]] = True
                out["%s__fast%d" % (case, t)] = np.packbits(mask.reshape(-1))
            a_img, pts, _ = skg.angle_input(ob, img)
            out["%s__angle_sha" % case] = np.array(skg.digest(a_img, pts))
            out["%s__angle" % case] = probe("angle", a_img, pts).astype(np.float64)
            blurred, pts, ang, _ = skg.desc_input(ob, img)
            out["%s__desc_sha" % case] = np.array(skg.digest(blurred, pts, ang))
            out["%s__desc" % case] = np.packbits(probe("desc", blurred, pts, ang).astype(np.uint8), axis=1, bitorder="little")
            print(case, {k: v.shape for k, v in out.items() if k.startswith(case + "__")})
    skg.GOLD.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(skg.GOLD, **out)
    print("wrote", skg.GOLD.relative_to(ROOT), skg.GOLD.stat().st_size, "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
