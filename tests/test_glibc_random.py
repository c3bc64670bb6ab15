"""csrc/vsf_glibc_random.h -- the one statement of glibc's rand() that the ObserveImage queue's colour kernel, its host side and
the host classes share -- against the system's C library (tests/cpp/test_glibc_random.cc: srandom / random for seeds 0, 1,
2, 7, 4242, 0xFFFFFFFF, 100 000 draws each; the unrolled block the kernel runs against the plain draw), plain and under
ASan / UBSan; and the packed colours against draw_ref.rand_colours fed by the C library's rand()."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
SRC = ROOT / "tests" / "cpp" / "test_glibc_random.cc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]


def _build(tmp_path, flags):
    exe = tmp_path / "test_glibc_random"
    r = subprocess.run(["g++", "-O1", "-std=c++17", *flags, "-o", str(exe), str(SRC)], capture_output=True, text=True)
    if flags and r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("no sanitizer runtime in this toolchain")
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("flags", [[], SAN])
def test_header_equals_libc(tmp_path, flags):
    p = subprocess.run([str(_build(tmp_path, flags))], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok 600000 draws"), (p.stdout, p.stderr[-2000:])


@pytest.mark.parametrize("seed", [1, 7, 4242])
def test_packed_colours_are_draw_refs(tmp_path, seed):
    import draw_ref
    exe = _build(tmp_path, [])
    n = 500
    p = subprocess.run([str(exe), "colours", str(seed), str(n)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    got = [int(x) for x in p.stdout.split()]
    libc = C.CDLL("libc.so.6")
    libc.srand(seed)
    want = [c0 | (c1 << 8) | (c2 << 16) for c0, c1, c2 in draw_ref.rand_colours(libc.rand, n)]
    assert got == want
