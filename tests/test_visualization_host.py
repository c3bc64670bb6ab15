"""What the reference's driver publishes to RViz, on the CPU (host/slam_visualization.h, host/slam_to_ros.h SerializeMarker /
SerializeMarkerArray, csrc/vsf_world_points.h) as a stand-alone program (tests/cpp/test_visualization.cc): a Marker with two
points and a MarkerArray of two markers against bytes written out by hand; AddPoseGraph on a three-node problem with a factor
that skips a node and one that names a missing node; the predicate table of AddFeaturePoints under the identity and a
non-trivial pose.  Once plainly, once under AddressSanitizer and UBSan.  And the two md5sums beside the serialisers follow the
field lists of tools/ros_md5.py."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = str(ROOT / "tests" / "cpp" / "test_visualization.cc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_visualization(tmp_path, flags):
    exe = tmp_path / "test_visualization"
    # (-ffp-contract=off: the rule of csrc/vsf_world_points.h for every translation unit that includes it)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-o", str(exe), SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])


def test_marker_md5sums_follow_the_field_lists():
    sys.path.insert(0, str(ROOT / "tools"))
    import ros_md5
    marker, array = ros_md5.marker_md5s()  # (table() inside asserts the known sums: Point, Quaternion, Pose, Header, ColorRGBA)
    header = (ROOT / "vision_slam_frontend_amd" / "host" / "slam_to_ros.h").read_text()
    found = dict(re.findall(r'k(Marker\w*)Md5 = "([0-9a-f]{32})"', header))
    assert found == {"Marker": marker, "MarkerArray": array}
    # the array's md5 text carries the marker's md5sum; the marker's starts with its constants, in the order of the .msg
    assert ros_md5.md5_text("visualization_msgs/MarkerArray") == "%s markers" % marker
    text = ros_md5.md5_text("visualization_msgs/Marker").splitlines()
    assert text[0] == "uint8 ARROW=0" and text[15] == "uint8 DELETEALL=3" and text[16].endswith(" header") and len(text) == 31
