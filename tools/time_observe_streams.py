"""Aggregate throughput of the ObserveImage queue fed by S independent frame streams (vsf_observe_set_streams).

Round-robin submission with at most `--per-stream` (4) uncollected frames per stream, i.e. a queue of depth 4 S: what a
machine that serves S cameras has waiting.  640x480, 2000 features by default.  Prints one JSON line per run:
aggregate frames/s, the largest batch, batches, batches that carried more than one stream.

  --streams 8            S streams through ONE context (one shared queue)
  --streams 8 --separate S contexts of one stream each, run one after the other (what S cameras cost without streams)
  --streams 1 --depth 32 the single-stream queue at another depth (the yardstick: runs on a library without streams too)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _run(capi, frames, calibs, n_streams, depth, per_stream_frames, warm, life, nfeatures, thread):
    """One context, n_streams streams, `depth` uncollected frames at most; returns (seconds, frames, stats)."""
    L = capi.lib()
    h, w = frames.shape[2], frames.shape[3]
    batch = min(depth, 128)
    ctx = capi.Context(capi.default_params(w, h, max_images=2 * batch, nfeatures=nfeatures))
    try:
        ctx.set_option(capi.OPT_OBSERVE_THREAD, thread)
        ctx.observe_configure(depth, 0, 0)
        has_streams = hasattr(ctx, "observe_set_streams")
        if n_streams > 1 or has_streams:
            ctx.observe_set_streams(n_streams)
        ptr = [(frames[i, 0].ctypes.data, frames[i, 1].ctypes.data) for i in range(len(frames))]
        bp = float(np.float32(0.3))
        ticket, view, nbytes = C.c_int64(), C.c_void_p(), C.c_size_t()
        pending = []
        total = n_streams * (warm + per_stream_frames)
        t0 = None
        for g in range(total):
            if g == n_streams * warm:  # the clock starts on an empty queue
                while pending:
                    assert L.vsf_observe_collect_view(ctx._h, pending.pop(0), C.byref(view), C.byref(nbytes)) == capi.VSF_OK
                t0 = time.perf_counter()
            s, k = g % n_streams, g // n_streams
            if len(pending) == depth:
                assert L.vsf_observe_collect_view(ctx._h, pending.pop(0), C.byref(view), C.byref(nbytes)) == capi.VSF_OK
            left, right = ptr[(k + 3 * s) % len(frames)]
            if has_streams:
                st = L.vsf_observe_submit_stream(ctx._h, s, left, right, w, h, w, C.byref(calibs[s]), bp, life, C.byref(ticket))
            else:
                st = L.vsf_observe_submit(ctx._h, left, right, w, h, w, C.byref(calibs[s]), bp, life, C.byref(ticket))
            assert st == capi.VSF_OK, st
            pending.append(ticket.value)
        while pending:
            assert L.vsf_observe_collect_view(ctx._h, pending.pop(0), C.byref(view), C.byref(nbytes)) == capi.VSF_OK
        dt = time.perf_counter() - t0
        return dt, n_streams * per_stream_frames, ctx.observe_stats()
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--per-stream", type=int, default=4, help="uncollected frames per stream at most")
    ap.add_argument("--depth", type=int, default=0, help="queue depth (0: streams x per-stream)")
    ap.add_argument("--frames", type=int, default=0, help="timed frames per stream (0: about 4096 in all)")
    ap.add_argument("--warmup", type=int, default=0, help="untimed frames per stream (0: a quarter of --frames)")
    ap.add_argument("--separate", action="store_true", help="one context per stream, one after the other")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--frame-life", type=int, default=5)
    ap.add_argument("--thread", type=int, default=0, help="VSF_OPT_OBSERVE_THREAD")
    ap.add_argument("--label", default="")
    a = ap.parse_args()

    import torch  # noqa: F401  (before libvsf_hip.so: the other order leaves torch without GPUs)

    from vision_slam_frontend_amd import capi, frontend, synth
    S = a.streams
    depth = a.depth or S * a.per_stream
    per = a.frames or max(64, 4096 // S)
    warm = a.warmup or max(8, per // 4)
    frames = synth.bench_batch(16, a.width, a.height)
    calibs = []
    for s in range(S):  # every stream its own calibration (a shared batch then reads them through the table)
        c = frontend.default_calibration()
        F = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0.01 * s]], np.float32)
        pr = c.get("projection_right").copy()
        pr[3] *= 1.0 + 0.01 * s
        calibs.append(c.set("fundamental", F).set("projection_right", pr))
    if a.separate:
        dt = n = 0
        stats = {}
        for s in range(S):
            d, m, stats = _run(capi, frames, [calibs[s]], 1, a.per_stream, per, warm, a.frame_life, a.nfeatures, a.thread)
            dt, n = dt + d, n + m
    else:
        dt, n, stats = _run(capi, frames, calibs, S, depth, per, warm, a.frame_life, a.nfeatures, a.thread)
    print(json.dumps({"label": a.label, "mode": "separate" if a.separate else "shared", "streams": S,
                      "depth": a.per_stream if a.separate else depth, "frames": n, "seconds": round(dt, 4),
                      "frames_per_s": round(n / dt, 1), "max_batch": stats.get("max_batch"), "batches": stats.get("batches"),
                      "multi_stream_batches": stats.get("multi_stream_batches", 0), "width": a.width, "height": a.height,
                      "nfeatures": a.nfeatures, "frame_life": a.frame_life}))


if __name__ == "__main__":
    main()
