"""sensor_msgs/CompressedImage as host/slam_to_ros.h writes it (the debug images as JPEG files): the wire bytes round-trip
(tests/cpp/test_ros_compressed_image.cc, also under ASan / UBSan), and the md5sum the header publishes is what tools/ros_md5.py
computes from the field lists -- the tool pins its rule on the md5sums every ROS-1 installation carries."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
SRC = ROOT / "tests" / "cpp" / "test_ros_compressed_image.cc"


def test_md5sum_is_computed_not_typed():
    import ros_md5
    header = (ROOT / "vision_slam_frontend_amd" / "host" / "slam_to_ros.h").read_text()
    found = re.findall(r'kCompressedImageMd5 = "([0-9a-f]{32})"', header)
    assert found == [ros_md5.compressed_image_md5()]
    assert ros_md5.md5_text("sensor_msgs/CompressedImage") == "%s header\nstring format\nuint8[] data" % ros_md5.md5("std_msgs/Header")
    assert ros_md5.md5_text("std_msgs/Header") == "uint32 seq\ntime stamp\nstring frame_id"
    assert len(ros_md5.table()) == 9  # (the package's own messages are what they were)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]])
def test_wire_round_trip(tmp_path, flags):
    exe = tmp_path / "test_ros_compressed_image"
    r = subprocess.run(["g++", "-O1", "-std=c++17", *flags, "-o", str(exe), str(SRC)], capture_output=True, text=True)
    if flags and r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("no sanitizer runtime in this toolchain")
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout, p.stderr[-2000:])
