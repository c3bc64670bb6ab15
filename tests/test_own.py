"""The owner template every device buffer, pinned buffer, event and stream of the library is an instance of (csrc/vsf_own.h),
with traits that count (tests/cpp/test_own.cc), under AddressSanitizer and UBSan: an empty owner releases nothing; moves
transfer; move assignment, alloc() and reset() release what was held exactly once; release() hands out without releasing; a
vector of owners through reallocations and a struct of owners assigned from a default-constructed one release every handle
once; at exit releases equal acquisitions."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "cpp" / "test_own.cc"


def test_owner_template(tmp_path):
    exe = tmp_path / "test_own"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-o", str(exe), str(SRC)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-2000:], p.stderr[-2000:])
