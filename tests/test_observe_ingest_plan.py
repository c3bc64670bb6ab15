"""The ingest plan of a batch of the ObserveImage queue (csrc/vsf_observe_plan.cc observe_ingest_plan: what every frame of the
batch is, the presence flags, the device ring's copies, the big-slot frames' uploads and resize runs, where the one demosaic and
the one ingest finish run) as a stand-alone program on the CPU (tests/cpp/test_observe_ingest_plan.cc): randomised batches at
depths 1 .. 1024 against a second spelling written frame by frame, and fixed cases written out by hand.  Once plainly, once
under AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRCS = [str(ROOT / "tests" / "cpp" / "test_observe_ingest_plan.cc"),
        str(ROOT / "vision_slam_frontend_amd" / "csrc" / "vsf_observe_plan.cc")]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_observe_ingest_plan(tmp_path, flags):
    exe = tmp_path / "test_observe_ingest_plan"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), *SRCS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])
