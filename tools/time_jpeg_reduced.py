#!/usr/bin/env python3
"""The reduced-size JPEG decode (IMREAD_REDUCED_GRAYSCALE_2) measured against full size, and the old paths against the parent
commit's library.  Every run is a process of its own under `timeout -k 10`; sides alternate, --runs (>= 3) per side; a run
that fails or runs out of time ends the measurement.  Records go to profiles/r12/jpeg_reduced.json.

  (a) decode   512 files of 1280 x 960 (8 distinct images, quality 85; baseline, then progressive) through
               vsf_imdecode_reduced_gray_batch at reduce 2, against the full-size decode of the same files by --parent-root
               (a built checkout of the parent commit; without it, by this library).  Images per second.
  (b) queue    frames/s of the ObserveImage queue into a 640 x 480 context from 1280 x 960 JPEGs at reduce 2, beside
               640 x 480 JPEGs at reduce 1, with the host's time inside a submit.
  (c) old      the full-size compressed queue and the raw queue, this library against --parent-root.

  python tools/time_jpeg_reduced.py [--parent-root DIR]      everything, then the JSON file
  python tools/time_jpeg_reduced.py --one decode|queue ...   one run in this process; prints one JSON line
"""
from __future__ import annotations

import argparse
import ctypes as C
import io
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
W, H = 640, 480


def _files(w, h, n, progressive):
    from PIL import Image

    from vision_slam_frontend_amd import synth
    base = synth.bench_batch(4, w, h, n_scenes=4).reshape(-1, h, w)
    distinct = []
    for img in base:
        b = io.BytesIO()
        Image.fromarray(img, "L").save(b, "JPEG", quality=85, progressive=progressive)
        distinct.append(np.frombuffer(b.getvalue(), np.uint8))
    return [distinct[i % len(distinct)] for i in range(n)]


def one(a):
    import torch  # (before libvsf_hip.so: the other order leaves torch without GPUs)

    if a.root:  # another checkout's package and library (the parent commit's, built there)
        sys.path.insert(0, str(Path(a.root).resolve()))
    from vision_slam_frontend_amd import capi, frontend
    assert Path(capi.__file__).resolve().is_relative_to(Path(a.root or ROOT).resolve())
    L = capi.lib()
    d = a.reduce
    if a.one == "decode":
        n = a.images
        files = _files(W * 2, H * 2, n, a.kind == "progressive")
        ow, oh = (W * 2 + d - 1) // d, (H * 2 + d - 1) // d
        ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in files])
        sizes = (C.c_size_t * n)(*[len(f) for f in files])
        dst = torch.zeros((n, oh, ow), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        with capi.Context(capi.default_params(W, H, max_images=2, nfeatures=2000)) as ctx:
            if d == 1:  # (the call the parent has too)
                call = lambda: L.vsf_imdecode_gray_batch(ctx._h, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), n, ow, oh,
                                                         C.c_void_p(dst.data_ptr()), ow * oh, ow)
            else:
                call = lambda: L.vsf_imdecode_reduced_gray_batch(ctx._h, C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), n, d,
                                                                 ow, oh, C.c_void_p(dst.data_ptr()), ow * oh, ow)
            for _ in range(2):
                assert call() == 0
            ctx.sync()
            host, t0 = 0.0, time.perf_counter()
            for _ in range(a.reps):
                h0 = time.perf_counter()
                assert call() == 0
                host += time.perf_counter() - h0
            ctx.sync()
            dt = (time.perf_counter() - t0) / a.reps
        print(json.dumps({"what": "decode", "kind": a.kind, "reduce": d, "root": "parent" if a.root else "this", "images": n,
                          "kb_per_file": round(sum(len(f) for f in files) / n / 1024, 1), "ms_per_call": round(dt * 1e3, 3),
                          "host_ms_per_call": round(host / a.reps * 1e3, 3), "images_per_s": round(n / dt, 1)}))
        return
    # ---- the queue ----
    calib = frontend.default_calibration().set("fundamental", np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32))
    bp = float(np.float32(0.3))
    if a.mode == "raw":
        from vision_slam_frontend_amd import synth
        frames = synth.bench_batch(16, W, H)
        src = [(frames[i, 0].ctypes.data, frames[i, 1].ctypes.data) for i in range(len(frames))]
    else:
        files = _files(W * d, H * d, 32, False)
        src = [(files[2 * i], files[2 * i + 1]) for i in range(16)]
    with capi.Context(capi.default_params(W, H, max_images=2 * min(a.depth, 128), nfeatures=2000)) as ctx:
        ctx.observe_configure(a.depth, 0, 0)
        if a.mode != "raw":
            ctx.observe_set_compressed_cap(1 << 20)
        ticket, view, nbytes = C.c_int64(), C.c_void_p(), C.c_size_t()

        def submit(i):
            l, r = src[i % len(src)]
            if a.mode == "raw":
                return L.vsf_observe_submit(ctx._h, l, r, W, H, W, C.byref(calib), bp, 5, C.byref(ticket))
            if d == 1:  # (the call the parent has too)
                return L.vsf_observe_submit_compressed(ctx._h, l.ctypes.data, len(l), r.ctypes.data, len(r), 0, C.byref(calib), bp, 5,
                                                       C.byref(ticket))
            return L.vsf_observe_submit_compressed_reduced(ctx._h, 0, l.ctypes.data, len(l), r.ctypes.data, len(r), d, C.byref(calib),
                                                           bp, 5, C.byref(ticket))

        pending, t0, in_submit = [], None, 0.0
        for g in range(a.warmup + a.frames):
            if g == a.warmup:  # the clock starts on an empty queue
                while pending:
                    assert L.vsf_observe_collect_view(ctx._h, pending.pop(0), C.byref(view), C.byref(nbytes)) == 0
                t0, in_submit = time.perf_counter(), 0.0
            while len(pending) >= a.depth:
                assert L.vsf_observe_collect_view(ctx._h, pending.pop(0), C.byref(view), C.byref(nbytes)) == 0
            h0 = time.perf_counter()
            st = submit(g)
            in_submit += time.perf_counter() - h0
            assert st == 0, st
            pending.append(ticket.value)
        while pending:
            assert L.vsf_observe_collect_view(ctx._h, pending.pop(0), C.byref(view), C.byref(nbytes)) == 0
        dt = time.perf_counter() - t0
    print(json.dumps({"what": "queue", "mode": a.mode, "reduce": d, "root": "parent" if a.root else "this", "frames": a.frames,
                      "frames_per_s": round(a.frames / dt, 1), "submit_us_per_frame": round(in_submit / a.frames * 1e6, 2)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", choices=["decode", "queue"])
    ap.add_argument("--root", default="", help="--one: another checkout (built) than this one to import the package from")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit")
    ap.add_argument("--kind", choices=["baseline", "progressive"], default="baseline")
    ap.add_argument("--mode", choices=["raw", "compressed"], default="compressed")
    ap.add_argument("--reduce", type=int, default=2)
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=512)
    ap.add_argument("--depth", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=90, help="seconds a run may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r12" / "jpeg_reduced.json"))
    a = ap.parse_args()
    if a.one:
        return one(a)
    parent = a.parent_root

    def run(args):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, "--images", str(a.images), "--reps", str(a.reps),
               "--frames", str(a.frames), "--warmup", str(a.warmup), "--depth", str(a.depth)] + args
        # (a run that fails or runs out of time ends the measurement: nothing more is started on the GPU behind it)
        r = subprocess.run(cmd, capture_output=True, text=True, check=True)
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        return json.loads(line)

    def sides(name, what, this_args, other_args, other_name, key):
        runs = {"this": [], other_name: []}
        for _ in range(max(a.runs, 3)):
            runs[other_name].append(run(other_args))
            runs["this"].append(run(this_args))
        rec = {"what": what, "median": {s: statistics.median(r[key] for r in v) for s, v in runs.items()},
               "spread_" + other_name: [min(r[key] for r in runs[other_name]), max(r[key] for r in runs[other_name])], "runs": runs}
        record[name] = rec
        print(name, json.dumps(rec["median"]), flush=True)

    record = {}
    plib = ["--root", parent] if parent else []
    who = "parent" if parent else "this_full_size"
    for kind in ("baseline", "progressive"):
        sides("decode_" + kind, "512 %s files of 1280x960: reduce 2 (this commit) against the full-size decode (%s); images/s"
              % (kind, who), ["--one", "decode", "--kind", kind, "--reduce", "2"],
              ["--one", "decode", "--kind", kind, "--reduce", "1"] + plib, who, "images_per_s")
    sides("queue_reduced_vs_full", "ObserveImage queue into 640x480: 1280x960 JPEGs at reduce 2 (this) beside 640x480 JPEGs at "
          "reduce 1; frames/s", ["--one", "queue", "--reduce", "2"], ["--one", "queue", "--reduce", "1"], "full_size", "frames_per_s")
    if parent:
        sides("old_compressed_queue", "640x480 JPEGs through vsf_observe_submit_compressed: this commit against the parent; frames/s",
              ["--one", "queue", "--reduce", "1"], ["--one", "queue", "--reduce", "1"] + plib, "parent", "frames_per_s")
        sides("old_raw_queue", "raw 640x480 frames through vsf_observe_submit: this commit against the parent; frames/s",
              ["--one", "queue", "--mode", "raw", "--reduce", "1"], ["--one", "queue", "--mode", "raw", "--reduce", "1"] + plib,
              "parent", "frames_per_s")
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
