"""Which blurred pyramid a call's blur writes and which release it waits for and records (csrc/vsf_blur_plan.h, one plain
function the host code and this test share), on the CPU: tests/cpp/test_blur_plan.cc issues call sequences -- early
throughout, the fork beside FAST throughout, the option toggled, small calls, calls on a stream of their own and two-lane
calls in between, every sequence of up to 7 calls, random ones of 64 -- onto a model of the context's streams and checks at
every call that no blur writes a buffer a queued reader has not released and that the descriptors read what their own blur
wrote.  Once plainly, once under AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_blur_plan.cc"


def _run(tmp_path, name, flags):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), str(SRC)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])


def test_call_sequences(tmp_path):
    _run(tmp_path, "test_blur_plan", [])


def test_call_sequences_under_sanitizers(tmp_path):
    _run(tmp_path, "test_blur_plan_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
