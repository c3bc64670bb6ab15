"""The arithmetic of one batch of the ObserveImage queue with streams (csrc/vsf_observe_plan.cc: which descriptor set every
frame goes to, the pair list, the table of distinct calibrations, the cuts) as a stand-alone program on the CPU
(tests/cpp/test_observe_plan.cc): one stream reproduces the closed forms the queue used before it had streams; several
streams with rings that wrap, at frame_life 1 and at the largest window; duplicate and distinct calibrations; a cut at a
per-stream change of parameters and nowhere else.  Once plainly, once under AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRCS = [str(ROOT / "tests" / "cpp" / "test_observe_plan.cc"), str(ROOT / "vision_slam_frontend_amd" / "csrc" / "vsf_observe_plan.cc")]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_observe_plan(tmp_path, flags):
    exe = tmp_path / "test_observe_plan"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), *SRCS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])
