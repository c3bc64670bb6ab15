"""The slot arithmetic of device-resident frames in the ObserveImage queue (csrc/vsf_observe_plan.cc: the span of a
multi-frame submit in the ring, the split of a batch into raw, compressed and device runs with the wrap of the ring) as a
stand-alone program on the CPU (tests/cpp/test_observe_device_plan.cc): randomised kinds, depths 1 .. 1024, wraps.  Once
plainly, once under AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRCS = [str(ROOT / "tests" / "cpp" / "test_observe_device_plan.cc"),
        str(ROOT / "vision_slam_frontend_amd" / "csrc" / "vsf_observe_plan.cc")]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_observe_device_plan(tmp_path, flags):
    exe = tmp_path / "test_observe_device_plan"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), *SRCS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])
