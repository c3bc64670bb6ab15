#!/usr/bin/env python3
"""Throughput of bag_extract on the device: 512 files of 640x480 per vsf_bag_extract_batch call (host memory in, host memory out),
    bayer_gray   one-component JPEG files on a "bayer_rggb8" topic (the reference's own camera): gray decode, demosaic, colour encode
    colour420    4:2:0 colour JPEG files on a plain topic: colour decode, colour encode
    colour420_bayer  the same files on a Bayer topic: colour decode, channel 0, demosaic, colour encode
the demosaic kernel alone (vsf_to_bgr_batch_dev on 512 mosaics resident in HBM: source + destination bytes over its time, device
events around back-to-back launches), and the chain of the tests' references on ONE host core -- the system's libjpeg reading
the file (tests/jpeg_ref_bgr.py), the numpy demosaic (tests/bayer_bgr_ref.py), libjpeg writing the file (tests/jpeg_enc_ref.py).
That chain is no OpenCV and no tuned host program: it is a LOWER BOUND for what a host implementation does per core.
    python tools/time_bag_extract.py [n_images]
prints one JSON line."""
import ctypes as C
import io
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch
from PIL import Image

import bayer_bgr_ref as br
import jpeg_enc_ref
import jpeg_ref_bgr
from vision_slam_frontend_amd import capi, synth

N = int(sys.argv[1]) if len(sys.argv) > 1 else 512
W, H = 640, 480
REPS = 5
RGGB = 1
dev = torch.device("cuda", 0)
base = synth.bench_batch(16, W, H, n_scenes=4).reshape(-1, H, W)


def jpeg_of(img, mode, **opts):
    b = io.BytesIO()
    Image.fromarray(img, mode).save(b, "JPEG", **opts)
    return b.getvalue()


gray_files = [jpeg_of(base[k], "L", quality=90) for k in range(len(base))]
colour_files = [jpeg_of(np.dstack([base[k], base[(k + 1) % len(base)], base[(k + 5) % len(base)]]), "RGB", quality=85, subsampling=2)
                for k in range(len(base))]
out = {"what": "vsf_bag_extract_batch, %d files of %dx%d per call, quality 95" % (N, W, H), "n_images": N, "reps": REPS, "cases": []}
ctx = capi.Context(capi.default_params(64, 64, max_images=2, nfeatures=100))


def reference(data, bayer):
    img = jpeg_ref_bgr.imdecode_bgr(data, W, H)[1]
    if bayer:
        img = br.bayer_to_bgr(img[..., 0], RGGB)
    return jpeg_enc_ref.imencode(img, 95)


CAP = int(capi.lib().vsf_jpeg_encode_capacity(W, H, 3))
home = np.zeros((N, CAP), np.uint8)  # the caller's slots, allocated once (the first call touches their pages)
home_bytes = np.zeros(N, np.int32)
for name, pool, bayer in (("bayer_gray", gray_files, RGGB), ("colour420", colour_files, 0), ("colour420_bayer", colour_files, RGGB)):
    files = [pool[i % len(pool)] for i in range(N)]
    st, got = ctx.bag_extract_batch(files, W, H, bayer, 0)  # (through the Python wrapper once: the scratch grows here)
    assert st == capi.VSF_OK
    for k in range(2):  # the bytes are the reference chain's
        assert got[k] == reference(pool[k], bayer), "%s: file %d differs from the reference chain" % (name, k)
    # the C call itself, on arrays that exist before the clock starts
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    ptrs = (C.c_void_p * N)(*[b.ctypes.data for b in bufs])
    sizes = (C.c_size_t * N)(*[len(b) for b in bufs])
    call = lambda: capi.lib().vsf_bag_extract_batch(ctx._h, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), N, W, H, bayer, 0,  # noqa: E731
                                                    home.ctypes.data_as(C.c_void_p), CAP, home_bytes.ctypes.data_as(C.c_void_p))
    assert call() == capi.VSF_OK
    assert home[1, :home_bytes[1]].tobytes() == got[1]
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        st = call()
        times.append(time.perf_counter() - t0)
        assert st == capi.VSF_OK
    t0 = time.perf_counter()
    for k in range(8):
        reference(pool[k], bayer)
    ref_rate = 8 / (time.perf_counter() - t0)
    dt = statistics.median(times)
    out["cases"].append({"case": name, "kb_per_file_in": sum(map(len, files)) / N / 1024, "kb_per_file_out": float(home_bytes.sum()) / N / 1024,
                         "images_per_s": N / dt, "ms_per_call_median": dt * 1e3, "ms_per_call_all": [t * 1e3 for t in times],
                         "reference_chain_one_core_images_per_s": ref_rate})

# where a call's time goes: the same three stages by hand for the bayer_gray files, files up and NOTHING home (the files stay in
# device memory) -- the difference to the composed call is the way home: the files through pinned memory into the caller's slots
s = torch.cuda.Stream(device=dev)
ctx.set_stream(s.cuda_stream)
files = [gray_files[i % len(gray_files)] for i in range(N)]
cap = CAP
d_mosaic = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
d_bgr = torch.zeros((N, H, 3 * W), dtype=torch.uint8, device=dev)
d_files = torch.zeros((N, cap), dtype=torch.uint8, device=dev)
d_sizes = torch.zeros(N, dtype=torch.int32, device=dev)
torch.cuda.synchronize()


def by_hand():
    ctx.imdecode_gray_batch(files, W, H, d_mosaic.data_ptr(), W * H, W)
    assert ctx.to_bgr_batch_dev(d_mosaic.data_ptr(), N, W, H, RGGB, W * H, W, d_bgr.data_ptr(), 3 * W * H, 3 * W) == capi.VSF_OK
    ctx.jpeg_encode_batch_dev(d_bgr.data_ptr(), N, W, H, 3, 3 * W * H, 3 * W, 95, d_files.data_ptr(), cap, d_sizes.data_ptr())
    assert ctx.sync() == capi.VSF_OK


by_hand()
times = []
for _ in range(REPS):
    t0 = time.perf_counter()
    by_hand()
    times.append(time.perf_counter() - t0)
out["bayer_gray_by_hand_nothing_home"] = {"ms_per_call_median": statistics.median(times) * 1e3, "ms_per_call_all": [t * 1e3 for t in times]}
del d_mosaic, d_bgr, d_files, d_sizes

# the demosaic kernel alone: N mosaics in HBM, 20 launches between two events, five times
mosaics = torch.from_numpy(np.stack([base[i % len(base)] for i in range(N)])).to(dev)
bgr = torch.zeros((N, H, 3 * W), dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
run = lambda: ctx.to_bgr_batch_dev(mosaics.data_ptr(), N, W, H, RGGB, W * H, W, bgr.data_ptr(), 3 * W * H, 3 * W)  # noqa: E731
assert run() == capi.VSF_OK and ctx.sync() == capi.VSF_OK
want = br.bayer_to_bgr(base[1], RGGB)
assert np.array_equal(bgr[1].cpu().numpy().reshape(H, W, 3), want)
LAUNCHES = 20
per_launch = []
for _ in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(LAUNCHES):
        run()
    e1.record(s)
    e1.synchronize()
    per_launch.append(e0.elapsed_time(e1) / LAUNCHES)
us = statistics.median(per_launch) * 1e3
out["demosaic_kernel"] = {"us_per_launch_median": us, "us_per_launch_all": [t * 1e3 for t in per_launch],
                          "bytes_per_launch": 4 * N * W * H, "tb_per_s": 4 * N * W * H / (us * 1e-6) / 1e12,
                          "note": "source (1 B) + destination (3 B) per pixel over the kernel's time; the working set (%.0f MB) is larger than the 256 MB last-level cache"
                                  % (4 * N * W * H / 1e6)}
ctx.close()
print(json.dumps(out))
