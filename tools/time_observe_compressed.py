"""Frames per second of the reference's driver loop (slam_frontend_main.cc:98-133, 271-328) fed from N JPEG payloads held in
host memory, through slam::Frontend with the queue on (pipelined; depth 256, 128 frames per batch, as tools/time_frontend.py
`queued`), driven from C++ with no Python between the calls (vsfh_time_sequence / vsfh_time_compressed_sequence):

  raw         ObserveImage on images decoded BEFORE the clock starts (what tools/time_frontend.py measures)
  compressed  ObserveCompressedImage: the payloads go into the queue, the GPU decodes them inside the batch
  host        decode-then-observe: the system's libjpeg (tests/jpeg_ref.py, driven as cv::imdecode drives it; its C code,
              JSIMD_FORCENONE, so this is a LOWER bound of what a SIMD libjpeg-turbo on the same core would do) decodes both
              images of a frame on the caller's thread, then ObserveImage

640x480, 2000 features, baseline JPEG quality 85 of the synthetic stereo stream; `--runs` runs each (default 3) on a Frontend
of its own; prints frames/s and the host's microseconds per frame inside the calls, and with --json one record with the
median and every run.

    python tools/time_observe_compressed.py [--frames 3232] [--runs 3] [--quality 85] [--json]"""
from __future__ import annotations

import argparse
import ctypes as C
import io
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from vision_slam_frontend_amd import frontend, synth  # noqa: E402

F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)


def payloads(width, height, n, quality):
    from PIL import Image
    sc = synth.Scene(width, height)
    files = []
    for f in range(n):
        for eye in (0, 1):
            b = io.BytesIO()
            Image.fromarray(sc.render(f, eye), "L").save(b, "JPEG", quality=quality)
            files.append(b.getvalue())
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3232)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--sources", type=int, default=16)
    ap.add_argument("--modes", default="raw,compressed,host")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    import jpeg_ref
    w, h = 640, 480
    files = payloads(w, h, a.sources, a.quality)
    blob = np.frombuffer(b"".join(files), np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.uint64)
    decoded = np.stack([jpeg_ref.imdecode_gray(f, w, h)[1] for f in files]).reshape(a.sources, 2, h, w) \
        if jpeg_ref.available() else None
    L = frontend.lib()
    L.vsfh_time_compressed_sequence.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.vsfh_time_compressed_sequence.restype = C.c_double
    record = {}
    for mode in a.modes.split(","):
        if mode in ("raw", "host") and decoded is None:
            print("%-10s skipped: the system's libjpeg is not loadable" % mode)
            continue
        runs = []
        for _ in range(a.runs):
            fe = frontend.Frontend(w, h, nfeatures=a.nfeatures, fundamental=F_RECT)
            fe.set_pipelined(True)
            if mode == "raw":
                fps, mean_ms, worst_ms = fe.time_sequence(decoded, a.frames, warm=32)
            else:
                fn = C.cast(jpeg_ref._load().jpeg_ref_gray, C.c_void_p) if mode == "host" else None
                mean, worst = C.c_double(), C.c_double()
                fps = L.vsfh_time_compressed_sequence(fe._h, blob.ctypes.data, offsets.ctypes.data, a.sources, 0, w, h, a.frames,
                                                      32, fn, C.byref(mean), C.byref(worst))
                if fps < 0:
                    raise RuntimeError("%s: the loop failed, status %d" % (mode, fe.last_status))
                mean_ms, worst_ms = mean.value, worst.value
            runs.append((float(fps), 1e3 * float(mean_ms), 1e3 * float(worst_ms)))
            fe.close()
        fps = sorted(r[0] for r in runs)
        us = sorted(r[1] for r in runs)
        print("%-10s %7.0f frames/s (runs: %s), host %.1f us per frame inside the calls (runs: %s)" %
              (mode, fps[len(fps) // 2], " ".join("%.0f" % v for v in fps), us[len(us) // 2], " ".join("%.1f" % v for v in us)))
        record[mode] = {"frames_per_s": fps[len(fps) // 2], "runs": fps, "host_us_per_frame": us[len(us) // 2], "host_us_runs": us}
    if a.json:
        print(json.dumps({"what": "slam::Frontend fed from JPEG payloads in host memory, 640x480, %d features, depth 256 / 128 per "
                                  "batch, baseline JPEG quality %d, mean file %d bytes (tools/time_observe_compressed.py)" %
                                  (a.nfeatures, a.quality, int(np.mean([len(f) for f in files]))),
                          "frames": a.frames, "results": record}))


if __name__ == "__main__":
    main()
