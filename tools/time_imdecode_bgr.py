#!/usr/bin/env python3
"""Throughput of the colour ingest: a batch of 640x480 colour files -- JPEG 4:2:0 and 4:4:4 in one scan, progressive 4:2:0,
PNG RGB, all written by PIL from the bench's synthetic scenes (three of them as the three channels) -- through
vsf_imdecode_bgr_batch, the gray read of the SAME files through vsf_imdecode_gray_batch in the same session, and the reference
library's colour read (tests/jpeg_ref_bgr.py, tests/png_ref_bgr.py) on one core: a lower bound for a host decoder.  One set
per process:
    python tools/time_imdecode_bgr.py SET [n_images]      SET: jpeg420 | jpeg444 | jpegprog | pngrgb
prints one JSON line.  The finishing kernel's own time comes from a kernel trace of the same command."""
import ctypes as C
import io
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch
from PIL import Image

from vision_slam_frontend_amd import capi, synth

SETS = {"jpeg420": ("JPEG", dict(quality=85, subsampling=2)), "jpeg444": ("JPEG", dict(quality=85, subsampling=0)),
        "jpegprog": ("JPEG", dict(quality=85, subsampling=2, progressive=True)), "pngrgb": ("PNG", dict(compress_level=6))}
name = sys.argv[1]
N = int(sys.argv[2]) if len(sys.argv) > 2 else 512
W, H = 640, 480
REPS = 5
fmt, opts = SETS[name]
dev = torch.device("cuda", 0)
base = synth.bench_batch(16, W, H, n_scenes=4).reshape(-1, H, W)
cache = {}
for k in range(len(base)):
    rgb = np.dstack([base[k], base[(k + 1) % len(base)], base[(k + 5) % len(base)]])
    b = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(b, fmt, **opts)
    cache[k] = b.getvalue()
files = [cache[i % len(base)] for i in range(N)]
bufs = [np.frombuffer(f, np.uint8) for f in files]
ptrs = (C.c_void_p * N)(*[b.ctypes.data for b in bufs])
sizes = (C.c_size_t * N)(*[len(b) for b in bufs])
ctx = capi.Context(capi.default_params(W, H, max_images=2, nfeatures=2000))
s = torch.cuda.Stream(device=dev)
ctx.set_stream(s.cuda_stream)
d = torch.zeros((N, H, 3 * W), dtype=torch.uint8, device=dev)
torch.cuda.synchronize()


def rate(fn_name, row_bytes):
    """-> (images / s, host milliseconds per call, status): the C call itself, REPS calls between two synchronisations."""
    fn = getattr(capi.lib(), fn_name)
    call = lambda: fn(ctx._h, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), N, W, H, C.c_void_p(d.data_ptr()),
                      row_bytes * H, row_bytes)
    st = call()
    if st != capi.VSF_OK:
        return None, None, st
    call()
    ctx.sync()
    t0 = time.perf_counter()
    host = 0.0
    for _ in range(REPS):
        h0 = time.perf_counter()
        assert call() == capi.VSF_OK
        host += time.perf_counter() - h0
    ctx.sync()
    dt = (time.perf_counter() - t0) / REPS
    return N / dt, host / REPS * 1e3, st


out = {"set": name, "n_images": N, "width": W, "height": H, "kb_per_file": sum(len(f) for f in files) / N / 1024, "reps": REPS}
out["colour_images_per_s"], out["colour_host_ms_per_call"], st = rate("vsf_imdecode_bgr_batch", 3 * W)
out["colour_status"] = int(st)
if st == capi.VSF_OK:   # the bytes are the reference's
    import jpeg_ref_bgr
    import png_ref_bgr
    got = d.cpu().numpy().reshape(N, H, W, 3)
    ref = jpeg_ref_bgr.imdecode_bgr if fmt == "JPEG" else png_ref_bgr.imdecode_bgr
    for k in range(len(base)):
        assert np.array_equal(got[k], ref(cache[k], W, H)[1]), "file %d differs from the reference" % k
    out["checked_against_reference"] = len(base)
out["gray_images_per_s"], out["gray_host_ms_per_call"], st = rate("vsf_imdecode_gray_batch", W)
assert st == capi.VSF_OK
ctx.close()
import jpeg_ref_bgr
import png_ref_bgr
ref = jpeg_ref_bgr.imdecode_bgr if fmt == "JPEG" else png_ref_bgr.imdecode_bgr
t0 = time.perf_counter()
for k in range(32):
    assert ref(files[k], W, H)[0] == 0
out["reference_one_core_images_per_s"] = 32 / (time.perf_counter() - t0)
# what the finishing kernel moves per call: a byte of luminance and the chroma samples in, three bytes out, per pixel
if fmt == "JPEG":
    chroma = 2.0 if opts["subsampling"] == 0 else 0.5
    out["finish_bytes_per_call"] = int(N * W * H * (1 + chroma + 3))
print(json.dumps(out))
