"""The pyramid's packing plan and cv::resize's coefficient formula as csrc/vsf_resize.h states them once for the host and
every kernel form (tests/cpp/test_pyramid_plan.cc): exact division by multiply-high for every lane of every wave, every
(strip, lane) produced once, at most 64 / R strips per wave, the tap-fetch lane below 64 -- for every band width 1..256,
R = 8 and 16 -- the packed / plain decision at the two model points, and the taps of four level sizes against the
definition evaluated in double precision."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_pyramid_plan.cc"


def test_plan_and_taps(tmp_path):
    exe = tmp_path / "test_pyramid_plan"
    # (no FMA contraction: the library is compiled that way, and the formula's float steps must round one by one)
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-o", str(exe), str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])
