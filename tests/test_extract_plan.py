"""The schedule of an extraction (csrc/vsf_extract_plan.h: the books, the decisions and the order of waits, records and
launches -- the host code issues it onto the GPU, this test onto a model), on the CPU: tests/cpp/test_extract_plan.cc drives
the real order function over call sequences -- early throughout, the fork beside FAST throughout, the options toggled, small
calls, calls on a stream of their own, two-lane calls, the tune call, pipelining off and on and batches of the queue in
between, every sequence of up to 7 calls, random ones of 64, each with and without the host wait vsf_set_option makes where
the options change -- onto a model of the context's streams and checks at every call
that no writer of a pyramid, candidate or blurred-pyramid buffer runs beside a queued reader of it, that every reader reads
what its own call wrote, and that each of three planners that are wrong on purpose is caught.  Once plainly, once under
AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_extract_plan.cc"


def _run(tmp_path, name, flags):
    exe = tmp_path / name
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, "-o", str(exe), str(SRC)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])


def test_call_sequences(tmp_path):
    _run(tmp_path, "test_extract_plan", [])


def test_call_sequences_under_sanitizers(tmp_path):
    _run(tmp_path, "test_extract_plan_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
