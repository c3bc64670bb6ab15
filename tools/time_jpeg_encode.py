#!/usr/bin/env python3
"""Throughput of the JPEG encoder alone: N images of 640x480 per vsf_jpeg_encode_batch_dev call (device to device), gray and BGR,
quality 95, against the same images through the system's libjpeg on ONE host core (tests/jpeg_enc_ref.py: the library as
installed, driven as cv::imencode(".jpg") drives it -- note that that binding switches libjpeg-turbo's SIMD routines off, so the
host figure is the C code's).  Writes one JSON object; with a path argument, into that file too.
    python tools/time_jpeg_encode.py [n_images] [out.json]
Then the ObserveImage queue at 640x480 / 2000 features / depth 256 (as tools/time_debug_images.py runs it) with the debug
images leaving as raw canvases and as JPEG files (FrontendConfig::debug_jpeg_quality_ = 95), in alternating runs on the same
box; --no-queue leaves that half out."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np
import torch

import jpeg_enc_ref as ref
from vision_slam_frontend_amd import capi, synth

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(ARGS[0]) if ARGS else 512
W, H, Q, REPS = 640, 480, 95, 5
dev = torch.device("cuda", 0)
gray = synth.bench_batch(8, W, H, n_scenes=4).reshape(-1, H, W)
result = {"what": "vsf_jpeg_encode_batch_dev alone, %d images of %dx%d per call, quality %d" % (N, W, H, Q), "cases": []}
ctx = capi.Context(capi.default_params(W, H, max_images=2, nfeatures=100))
for ch in (1, 3):
    base = gray if ch == 1 else np.stack([gray, np.roll(gray, 5, 1), np.roll(gray, 3, 2)], -1)
    imgs = np.ascontiguousarray(np.stack([base[i % len(base)] for i in range(N)]))
    stride = capi.jpeg_encode_capacity(W, H, ch)
    d_src = torch.from_numpy(imgs).to(dev)
    d_out = torch.zeros(N * stride, dtype=torch.uint8, device=dev)
    d_n = torch.zeros(N, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    run = lambda: ctx.jpeg_encode_batch_dev(d_src.data_ptr(), N, W, H, ch, W * H * ch, W * ch, Q, d_out.data_ptr(), stride,
                                            d_n.data_ptr())
    for _ in range(2):
        run()
    assert ctx.sync() == capi.VSF_OK
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        run()
        ctx.sync()
        times.append(time.perf_counter() - t0)
    sizes = d_n.cpu().numpy()
    first = d_out[:int(sizes[0])].cpu().numpy().tobytes()
    t0 = time.perf_counter()
    n_host = min(N, 32)
    host_files = [ref.imencode(imgs[i], Q) for i in range(n_host)]
    host = (time.perf_counter() - t0) / n_host
    assert first == host_files[0], "the device's file differs from libjpeg's"
    dt = float(np.median(times))
    case = {"channels": ch, "mean_file_bytes": float(sizes.mean()), "raw_bytes": W * H * ch, "ms_per_call_median": dt * 1e3,
            "ms_per_call_all": [t * 1e3 for t in times], "images_per_s": N / dt, "libjpeg_one_core_images_per_s": 1.0 / host,
            "libjpeg_simd": "off (JSIMD_FORCENONE, as the byte-exact reference is run)"}
    result["cases"].append(case)
    print("%d channel(s): %d images in %.2f ms = %.0f images/s (files of %.0f KB for %.0f KB raw); libjpeg on one core %.0f images/s"
          % (ch, N, dt * 1e3, N / dt, sizes.mean() / 1024, W * H * ch / 1024, 1.0 / host))
ctx.close()


def queued_fps(jpeg_quality: int, n_frames: int = 544, nfeatures: int = 2000, depth: int = 256):
    """tools/time_debug_images.py queued_fps with the debug images on, raw (0) or as files."""
    from vision_slam_frontend_amd import frontend
    sc = synth.Scene(640, 480)
    frames = np.stack([np.stack([sc.render(f, 0), sc.render(f, 1)]) for f in range(32)]).astype(np.uint8)
    F = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    fe = frontend.Frontend(640, 480, nfeatures=nfeatures, fundamental=F, debug_images=True, debug_jpeg_quality=jpeg_quality)
    fe.set_pipelined(True)
    fe.set_queue(depth, 0, 0)
    fps, mean_ms, _ = fe.time_sequence(frames, n_frames, warm=32)
    size = len(fe.last_debug_image_compressed(stereo=True) or b"") + len(fe.last_debug_image_compressed() or b"")
    fe.close()
    return fps, mean_ms, size


if "--no-queue" not in sys.argv[1:]:
    runs = {"raw_canvases": [], "jpeg_files_q95": []}
    file_bytes = 0
    for rep in range(3):  # alternating, so that a drift of the box shows in both
        for key, q in (("raw_canvases", 0), ("jpeg_files_q95", 95)):
            fps, ms, size = queued_fps(q)
            runs[key].append(fps)
            file_bytes = max(file_bytes, size)
            print("queue, debug images as %-14s run %d: %8.0f frames/s" % (key, rep, fps))
    result["queue"] = {"what": "ObserveImage queue, 640x480 / 2000 features / depth 256, debug images on; frames/s of alternating runs",
                       "frames_per_s": runs, "median": {k: float(np.median(v)) for k, v in runs.items()},
                       "bytes_home_per_frame": {"raw_canvases": 9 * 640 * 480, "jpeg_files_q95": file_bytes}}
print(json.dumps(result))
if len(ARGS) > 1:
    Path(ARGS[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(ARGS[1]).write_text(json.dumps(result, indent=1) + "\n")
