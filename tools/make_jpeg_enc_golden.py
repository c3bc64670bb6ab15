"""Writes tests/golden/jpeg_enc/*.jpg: the named inputs of tests/jpeg_enc_ref.py encoded by the system's libjpeg driven as
cv::imencode(".jpg") of OpenCV 3.2 drives it (tests/cpp/jpeg_enc_ref.c).  The GPU encoder must write the same files
(tests/test_gpu_jpeg_enc.py); tests/test_jpeg_enc_host.py checks that the library of the machine the tests run on still does."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import jpeg_enc_ref as ref  # noqa: E402


def main():
    assert ref.available(), "libjpeg.so.8 cannot be loaded"
    ref.GOLDEN.mkdir(parents=True, exist_ok=True)
    total = 0
    for name, content, w, h, ch, q in ref.golden_cases():
        data = ref.imencode(ref.make_input(content, w, h, ch), q)
        (ref.GOLDEN / (name + ".jpg")).write_bytes(data)
        total += len(data)
        print("%-28s %6d bytes  %s" % (name, len(data), ref.scan_stats(data)))
    print("%d files, %d bytes" % (len(ref.golden_cases()), total))


if __name__ == "__main__":
    main()
