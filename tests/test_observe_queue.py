"""The host threads of the ObserveImage queue (csrc/vsf_observe_queue.cc: the release policy, the tickets and the baton, the
launcher thread, the staging copy's helper) as a stand-alone program on the CPU with a fake GPU
(tests/cpp/test_observe_queue.cc).  Once plainly, once under AddressSanitizer and UBSan, once under ThreadSanitizer -- the
last with the clang++ that ships beside hipcc: g++ 11's ThreadSanitizer runtime does not know pthread_cond_clockwait and
reports races in a correct condition_variable::wait_for on the steady clock, which the launcher thread uses.  A hang fails
through the timeout."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRCS = [str(ROOT / "tests" / "cpp" / "test_observe_queue.cc"), str(ROOT / "vision_slam_frontend_amd" / "csrc" / "vsf_observe_queue.cc")]
BASE = ["-std=c++17", "-Wall", "-Werror", "-pthread"]


def rocm_clang():
    hipcc = Path(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")).resolve()
    for c in (hipcc.parent / "clang++", hipcc.parent.parent / "llvm" / "bin" / "clang++", hipcc.parent.parent / "lib" / "llvm" / "bin" / "clang++"):
        if c.exists():
            return str(c)
    return shutil.which("amdclang++")


def build_and_run(tmp_path, cxx, flags):
    exe = tmp_path / "test_observe_queue"
    r = subprocess.run([cxx, *BASE, *flags, "-o", str(exe), *SRCS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.rstrip().endswith("ok observe queue"), (p.stdout[-2000:], p.stderr[-2000:])


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_observe_queue(tmp_path, flags):
    build_and_run(tmp_path, "g++", flags)


def test_observe_queue_tsan(tmp_path):
    cxx = rocm_clang()
    empty = tmp_path / "empty.cc"
    empty.write_text("int main() { return 0; }\n")
    if cxx is None or subprocess.run([cxx, "-fsanitize=thread", "-o", str(tmp_path / "empty"), str(empty)],
                                     capture_output=True).returncode != 0:
        pytest.skip("no clang++ beside hipcc that links a ThreadSanitizer program")
    build_and_run(tmp_path, cxx, ["-O1", "-g", "-fsanitize=thread"])
