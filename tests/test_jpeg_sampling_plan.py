"""The host half of the JPEG decode on every sampling layout of jpeg_craft.sampling_cases() / sampling_refusals(), as a
stand-alone program on the CPU (tests/cpp/test_jpeg_sampling_plan.cc, linked with csrc/vsf_jpeg_host.cc and the rest of the
sanitizer build's sources): each file alone through vsf_jpeg_plan at reduce 1, 2, 4, 8 with and without force_serial, each
same-size batch through vsf_jpeg_host_check.  Once plainly, once under AddressSanitizer and UBSan; nothing is preloaded and
nothing is loaded into Python.  What is asserted: the statuses, max_luma_blocks from Python's own arithmetic, and that every
file reaches the decoder tests/test_gpu_jpeg_sampling.py names it for -- `base` files the parallel one (n_par == 1), multi-scan
and progressive files the scan-list one (n_prog == 1), force_serial none of the parallel one."""
import subprocess
from pathlib import Path

import pytest

import jpeg_craft as jc

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "vision_slam_frontend_amd" / "csrc"
SRCS = [str(ROOT / "tests" / "cpp" / "test_jpeg_sampling_plan.cc")] + \
       [str(CSRC / n) for n in ("vsf_jpeg_host.cc", "vsf_png_host.cc", "vsf_ingest_host.cc", "vsf_jpeg_enc_host.cc",
                                "vsf_png_enc_host.cc", "vsf_jpeg_host_check.cc")]
VSF_OK, VSF_ERR_INVALID_ARG, VSF_ERR_UNSUPPORTED = 0, 1, 4   # include/vsf.h


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan_ubsan"])
def test_jpeg_sampling_plan(tmp_path, flags):
    exe = tmp_path / "test_jpeg_sampling_plan"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        "-o", str(exe), *SRCS, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    good = jc.sampling_cases()
    bad = jc.sampling_refusals()
    every = [c + (None,) for c in good] + list(bad)
    lines = []
    for i, (name, data, w, h, factors, process, answer) in enumerate(every):
        (tmp_path / ("%03d.jpg" % i)).write_bytes(data)
        lines.append("%s %d %d %d" % (tmp_path / ("%03d.jpg" % i), w, h, int(answer is None)))
    (tmp_path / "manifest.txt").write_text("\n".join(lines) + "\n")
    p = subprocess.run([str(exe), str(tmp_path / "manifest.txt")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    out = p.stdout.splitlines()
    assert out[-1].startswith("ok jpeg sampling plan: %d files" % len(every)), out[-1]
    per_file = {}
    batches = []
    for line in out[:-1]:
        f = line.split()
        if f[0] == "file":
            per_file[tuple(int(t) for t in f[1:4])] = tuple(int(t) for t in f[4:])
        else:
            assert f[0] == "batch", line
            batches.append(tuple(int(t) for t in f[1:]))
    assert len(per_file) == 8 * len(every)
    for i, (name, data, w, h, factors, process, answer) in enumerate(every):
        for reduce in (1, 2, 4, 8):
            for serial in (0, 1):
                st, n_par, n_prog, max_luma, mcus_x, mcus_y = per_file[(i, reduce, serial)]
                label = "%s at 1/%d, force_serial %d" % (name, reduce, serial)
                if answer is not None:
                    assert st == (VSF_ERR_INVALID_ARG if answer == "invalid_arg" else VSF_ERR_UNSUPPORTED), label
                    continue
                assert st == VSF_OK, label
                h0, v0 = factors[0] if len(factors) > 1 else (1, 1)   # a lone component: one block per MCU
                assert (mcus_x, mcus_y) == (-(-w // (8 * h0)), -(-h // (8 * v0))), label
                assert max_luma == mcus_x * mcus_y * h0 * v0, label
                if process in ("base", "base_rst"):
                    assert (n_par, n_prog) == (0 if serial else 1, 0), label
                else:
                    assert (n_par, n_prog) == (0, 1), label
    sizes = sorted({(c[2], c[3]) for c in good})
    assert len(batches) == 2 * len(sizes)
    for w, h, n, serial, st, total in batches:
        assert st == VSF_OK and n == sum(1 for c in good if (c[2], c[3]) == (w, h)) and total > 0, (w, h, serial, st, total)
