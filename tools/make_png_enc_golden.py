#!/usr/bin/env python3
"""Writes tests/golden/png_enc/*.png: what the system's libpng, driven as cv::imencode(".png") of OpenCV 3.2 drives it
(tests/png_enc_ref.py), writes for the named inputs of png_enc_ref.golden_cases().  The GPU encoder is compared with these files
as well as with the library, so the test still bites where the library differs."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))

import png_enc_ref as ref  # noqa: E402

if __name__ == "__main__":
    assert ref.available(), "libpng16.so.16 cannot be loaded"
    ref.GOLDEN.mkdir(parents=True, exist_ok=True)
    for old in ref.GOLDEN.glob("*.png"):
        old.unlink()
    for name, content, w, h, ch in ref.golden_cases():
        data = ref.imencode(ref.make_input(content, w, h, ch))
        assert data == ref.model(ref.make_input(content, w, h, ch)), name
        (ref.GOLDEN / (name + ".png")).write_bytes(data)
        print("%-28s %6d bytes" % (name, len(data)))
