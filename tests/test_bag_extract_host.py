"""The host half of slam::BagExtract (host/bag_extract.h): the reference's file name (src/test/bag_extract.cc:81-87) and the
grouping of a topic's messages into vsf_bag_extract_batch calls, as a stand-alone program on the CPU
(tests/cpp/test_bag_extract_plan.cc) -- once plainly, once under AddressSanitizer and UBSan -- and the file name again through
the binding of libvsf_frontend.so, against the iostream rule restated here."""
import math
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_bag_extract_plan.cc"


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_bag_extract_plan(tmp_path, flags):
    exe = tmp_path / "test_bag_extract_plan"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])


def _setw_rule(output, count, index):
    # ss << output << "/image" << setfill('0') << setw(log(count)) << index << ".jpg": setw takes an int (truncation), and a
    # field narrower than its content is printed whole
    return "%s/image%s.jpg" % (output, str(index).rjust(int(math.log(count)), "0"))


def test_path_through_the_binding():
    from vision_slam_frontend_amd import frontend
    assert frontend.bag_extract_path("out", 8, 7) == "out/image07.jpg"
    assert frontend.bag_extract_path("out", 1000, 12) == "out/image000012.jpg"
    assert frontend.bag_extract_path("out", 3, 12) == "out/image12.jpg"
    for count in (1, 2, 3, 7, 8, 20, 21, 1000):
        for index in (0, 1, 9, 10, count - 1, 5 * count + 100, 123456789):
            assert frontend.bag_extract_path("/tmp/x y", count, index) == _setw_rule("/tmp/x y", count, index), (count, index)
