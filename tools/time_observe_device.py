"""Raw host submit against device submit through the ObserveImage queue, from the same pixels.

640x480, 2000 features, depth 256 (128 frames per batch), frame_life 5 by default.  The frames are ONE resident [N, 2, H, W]
uint8 tensor; the raw runs submit its host copy with vsf_observe_submit (staging copy + one upload per batch), the device
runs submit views of the tensor with vsf_observe_submit_dev (one launch per frame on torch's current stream, no host copy,
no PCIe transfer).  Three alternating runs of each, every run a process of its own under its own time limit; the medians,
all runs and the host's nanosecond counters (vsf_observe_stats: staging / submit launches, batch launches, waits) go to
profiles/r10/observe_device.json.

  python tools/time_observe_device.py              the alternating runs, then the JSON file
  python tools/time_observe_device.py --one device one run in this process; prints one JSON line
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def one(a):
    import torch  # (before libvsf_hip.so: the other order leaves torch without GPUs)

    from vision_slam_frontend_amd import capi, frontend, synth
    L = capi.lib()
    w, h, depth = a.width, a.height, a.depth
    frames = synth.bench_batch(16, w, h)
    resident = torch.from_numpy(frames).to("cuda:0")  # [N, 2, H, W]
    torch.cuda.synchronize()
    calib = frontend.default_calibration().set("fundamental", np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32))
    bp = float(np.float32(0.3))
    ctx = capi.Context(capi.default_params(w, h, max_images=2 * min(depth, 128), nfeatures=a.nfeatures))
    try:
        ctx.observe_configure(depth, 0, 0)
        ticket, view, nbytes = C.c_int64(), C.c_void_p(), C.c_size_t()
        host = [(frames[i, 0].ctypes.data, frames[i, 1].ctypes.data) for i in range(len(frames))]
        # (--per-call k: frame i of a call is resident frame (g + i) % N, as k calls of one would take them)
        k_call = a.per_call if a.one == "device" else 1
        dev = [(capi.VsfDevFrame * k_call)(*[capi.VsfDevFrame(resident[(i + j) % len(frames), 0].data_ptr(),
                                                              resident[(i + j) % len(frames), 1].data_ptr(), w, w)
                                             for j in range(k_call)]) for i in range(len(frames))]
        side = torch.cuda.Stream() if a.producer == "side" else None  # a producer with a stream of its own
        stream = C.c_void_p((side or torch.cuda.current_stream()).cuda_stream or None)
        tickets = (C.c_int64 * k_call)()

        def submit(i):
            if a.one == "raw":
                st = L.vsf_observe_submit(ctx._h, host[i][0], host[i][1], w, h, w, C.byref(calib), bp, a.frame_life, C.byref(ticket))
                assert st == capi.VSF_OK, st
                return [ticket.value]
            st = L.vsf_observe_submit_dev(ctx._h, 0, dev[i], k_call, capi.PIX_MONO8, stream, C.byref(calib), bp, a.frame_life, tickets)
            assert st == capi.VSF_OK, st
            return list(tickets)

        def collect(t):
            assert L.vsf_observe_collect_view(ctx._h, t, C.byref(view), C.byref(nbytes)) == capi.VSF_OK

        pending, t0, s0 = [], None, None
        for g in range(0, a.warmup + a.frames, k_call):
            if g == a.warmup:  # the clock starts on an empty queue
                while pending:
                    collect(pending.pop(0))
                s0, t0 = ctx.observe_stats(), time.perf_counter()
            while len(pending) + k_call > depth:
                collect(pending.pop(0))
            pending += submit(g % len(frames))
        while pending:
            collect(pending.pop(0))
        dt = time.perf_counter() - t0
        s1 = ctx.observe_stats()
    finally:
        ctx.close()
    per_frame = {k: round((s1[k] - s0[k]) / a.frames, 1) for k in ("copy_ns", "launch_ns", "wait_ns")}
    print(json.dumps({"mode": a.one, "frames": a.frames, "seconds": round(dt, 4), "frames_per_s": round(a.frames / dt, 1),
                      "host_ns_per_frame": per_frame, "batches": s1["batches"] - s0["batches"], "max_batch": s1["max_batch"],
                      "device_frames": s1["device_frames"], "device_commands": s1["device_commands"],
                      "device_ring_bytes": s1["device_ring_bytes"], "per_call": k_call, "producer": a.producer, "width": w, "height": h, "nfeatures": a.nfeatures,
                      "depth": depth, "frame_life": a.frame_life}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", choices=["raw", "device"], help="one run in this process")
    ap.add_argument("--runs", type=int, default=3, help="alternating runs of each mode")
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=1024)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--depth", type=int, default=256)
    ap.add_argument("--frame-life", type=int, default=5)
    ap.add_argument("--per-call", type=int, default=1, help="device runs: frames per vsf_observe_submit_dev call (divides --warmup)")
    ap.add_argument("--producer", choices=["current", "side"], default="current",
                    help="device runs: submit on torch's current stream (the default stream) or on a side stream")
    ap.add_argument("--key", default="device_vs_raw_submit", help="the record's name in the JSON file")
    ap.add_argument("--timeout", type=int, default=120, help="seconds a run may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r10" / "observe_device.json"))
    a = ap.parse_args()
    if a.one:
        return one(a)
    runs = {"raw": [], "device": []}
    passed = [sys.executable, __file__, "--frames", str(a.frames), "--warmup", str(a.warmup), "--width", str(a.width), "--height",
              str(a.height), "--nfeatures", str(a.nfeatures), "--depth", str(a.depth), "--frame-life", str(a.frame_life), "--per-call", str(a.per_call), "--producer",
              a.producer]
    for _ in range(a.runs):
        for mode in ("raw", "device"):
            # (a run that fails or runs out of time ends the measurement: nothing more is started on the GPU behind it)
            r = subprocess.run(passed + ["--one", mode], capture_output=True, text=True, timeout=a.timeout, check=True)
            runs[mode].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(r.stdout.strip().splitlines()[-1], flush=True)
    out = Path(a.out)
    record = json.loads(out.read_text()) if out.exists() else {}
    record[a.key] = {
        "what": "ObserveImage queue, %dx%d, %d features, depth %d: vsf_observe_submit of host images against "
                "vsf_observe_submit_dev of the same pixels resident in HBM (%d per call, on torch's %s stream); alternating "
                "runs, frames/s" % (a.width, a.height, a.nfeatures, a.depth, a.per_call, a.producer),
        "median_frames_per_s": {m: statistics.median(r["frames_per_s"] for r in runs[m]) for m in runs},
        "runs": runs,
    }
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record, indent=1) + "\n")
    print(json.dumps(record[a.key]["median_frames_per_s"]))


if __name__ == "__main__":
    main()
