#!/usr/bin/env python3
"""A declared input size per stream of the ObserveImage queue (vsf_observe_set_input_size), measured with a 640x480 context /
2000 features / depth 256 (128 frames per batch).  Each run is one process under its own time limit; the sides alternate (and
who goes first alternates too), behind one discarded process that warms the machine.

  old paths   the raw queue, the compressed queue (640x480 JPEG) and the device queue (8 frames per call): this library against
              --parent-root (a built checkout of the parent commit), four runs a side.  The condition: this commit's median
              is not below the parent's LOWEST run.
  report      1280x960 raw host frames, and separately device frames (8 per call), into the 640x480 context with the resize
              on the device -- against (a) the same queue fed frames already at 640x480, the ceiling, and (b) the resize on
              the caller's thread with the scalar restatement of cv::resize (the oracle's), then raw submit: a LOWER BOUND
              for a host resize (no SIMD, one thread), as the libjpeg figure of the reduced decode is.  The submitting
              thread's microseconds per frame in every mode.
  The resize kernel's own time comes from a profiler run of `--one big_dev` (kernel trace + stats, no counters): its bytes
  (source + destination, from the shapes) over that time as a share of the 8 TB/s HBM peak -- a kernel's share, not the queue's.

  python tools/time_observe_resize.py [--parent-root DIR] [--part old|report|all]     then the JSON file
  python tools/time_observe_resize.py --one MODE [--root DIR]                          one run, one JSON line"""
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
W, H, BW, BH, NF, DEPTH, BATCH, LIFE, PER_CALL = 640, 480, 1280, 960, 2000, 256, 128, 5, 8
MODES = ("raw", "jpeg", "dev", "big_raw", "big_dev", "host_resize")
HBM_PEAK = 8.0e12


def one(a):
    import torch  # (before libvsf_hip.so: the other order leaves torch without GPUs)

    sys.path.insert(0, str(Path(a.root).resolve()) if a.root else str(ROOT))
    from vision_slam_frontend_amd import capi, frontend, synth
    assert Path(capi.__file__).resolve().is_relative_to(Path(a.root or ROOT).resolve())
    L = capi.lib()
    calib = frontend.default_calibration().set("fundamental", np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32))
    bp = float(np.float32(0.3))
    mode = a.one
    big = mode in ("big_raw", "big_dev", "host_resize")
    fw, fh = (BW, BH) if big else (W, H)
    frames = synth.bench_batch(16, fw, fh)
    ticket, view, nbytes = C.c_int64(), C.c_void_p(), C.c_size_t()
    files = dev = None
    if mode == "jpeg":
        from PIL import Image

        def enc(img):
            b = io.BytesIO()
            Image.fromarray(img, "L").save(b, "JPEG", quality=90)
            return np.frombuffer(b.getvalue(), np.uint8)
        files = [(enc(frames[i, 0]), enc(frames[i, 1])) for i in range(len(frames))]
    if mode in ("dev", "big_dev"):
        dev = torch.from_numpy(frames).to("cuda:0")
        torch.cuda.synchronize()
        arr = (capi.VsfDevFrame * PER_CALL)()
        tickets = (C.c_int64 * PER_CALL)()
        stream = torch.cuda.current_stream(0).cuda_stream
    if mode == "host_resize":
        from oracle import binding as ob
        ob.lib()
    ctx = capi.Context(capi.default_params(W, H, max_images=2 * BATCH, nfeatures=NF))
    ctx.observe_configure(DEPTH, 0, 0)
    if mode in ("big_raw", "big_dev"):
        ctx.observe_set_input_size(0, BW, BH)
    pending, t0, in_submit = [], None, 0.0

    def collect():
        assert L.vsf_observe_collect_view(ctx._h, pending.pop(0), C.byref(view), C.byref(nbytes)) == 0

    step = PER_CALL if dev is not None else 1
    for g in range(0, a.warmup + a.frames, step):
        if g == a.warmup:  # the clock starts on an empty queue
            while pending:
                collect()
            t0, in_submit = time.perf_counter(), 0.0
        while len(pending) + step > DEPTH:
            collect()
        i = g % len(frames)
        h0 = time.perf_counter()
        if dev is not None:
            for k in range(PER_CALL):
                l, r = dev[(i + k) % len(frames), 0], dev[(i + k) % len(frames), 1]
                arr[k] = capi.VsfDevFrame(l.data_ptr(), r.data_ptr(), fw, fw)
            st = L.vsf_observe_submit_dev(ctx._h, 0, arr, PER_CALL, 0, C.c_void_p(stream or None), C.byref(calib), bp, LIFE, tickets)
            new = list(tickets)
        elif files is not None:
            l, r = files[i]
            st = L.vsf_observe_submit_compressed(ctx._h, l.ctypes.data, len(l), r.ctypes.data, len(r), 0, C.byref(calib), bp, LIFE,
                                                 C.byref(ticket))
            new = [ticket.value]
        else:
            l, r = frames[i, 0], frames[i, 1]
            if mode == "host_resize":  # (b): cv::resize on the caller's thread, then a frame like any other
                l, r = ob.resize_linear(l, W, H), ob.resize_linear(r, W, H)
            st = L.vsf_observe_submit(ctx._h, l.ctypes.data, r.ctypes.data, l.shape[1], l.shape[0], l.shape[1], C.byref(calib), bp,
                                      LIFE, C.byref(ticket))
            new = [ticket.value]
        in_submit += time.perf_counter() - h0
        assert st == 0, st
        pending += new
    while pending:
        collect()
    dt = time.perf_counter() - t0
    stats = ctx.observe_stats()
    ctx.close()
    assert stats.get("resized_frames", 0) == ((a.frames + a.warmup) if mode in ("big_raw", "big_dev") else 0)
    print(json.dumps({"mode": mode, "root": "parent" if a.root else "this", "frames": a.frames, "frames_per_s": round(a.frames / dt, 1),
                      "submit_us_per_frame": round(in_submit / a.frames * 1e6, 2)}))


def run_one(args, limit):
    p = subprocess.run([sys.executable, __file__] + args, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        raise SystemExit("run %s failed (%d): %s" % (args, p.returncode, p.stderr[-2000:]))
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(rec), flush=True)
    return rec


def sides(out, key, what, this_args, other_args, other_name, runs, limit):
    """`runs` runs a side, alternating; the medians, every run, and both sides' spreads."""
    got = {"this": [], other_name: []}
    for i in range(runs):  # (who goes first alternates too: a run may inherit something from the process before it)
        for who in (("this", other_name) if i % 2 == 0 else (other_name, "this")):
            got[who].append(run_one(this_args if who == "this" else other_args, limit))
    fps = {k: [r["frames_per_s"] for r in v] for k, v in got.items()}
    out[key] = {"what": what, "median": {k: statistics.median(v) for k, v in fps.items()},
                "spread": {k: [min(v), max(v)] for k, v in fps.items()},
                "submit_us_per_frame_median": {k: statistics.median(r["submit_us_per_frame"] for r in v) for k, v in got.items()},
                "runs": got}
    return out[key]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", choices=MODES)
    ap.add_argument("--frames", type=int, default=0, help="timed frames of a run (0: 4096; 1024 for the host resize)")
    ap.add_argument("--warmup", type=int, default=256)
    ap.add_argument("--root", default="", help="--one: another checkout (built) than this one to import the package from")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit")
    ap.add_argument("--part", choices=["old", "report", "all", "none"], default="all")
    ap.add_argument("--runs", type=int, default=4, help="runs a side of the old paths")
    ap.add_argument("--report-runs", type=int, default=3, help="runs a side of the report")
    ap.add_argument("--limit", type=int, default=240, help="seconds a run may take")
    ap.add_argument("--kernel-stats", default="", help="a profiler's kernel_stats.csv of a `--one big_dev` run to take the resize kernel's time from")
    ap.add_argument("--bench-dir", default="", help="a directory of bench.py result lines (this_*.json, parent_*.json) to record")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r14" / "observe_resize.json"))
    a = ap.parse_args()
    if a.one:
        a.frames = a.frames or (1024 if a.one == "host_resize" else 4096)
        return one(a)
    out_path = Path(a.out)
    out = json.loads(out_path.read_text()) if out_path.exists() else {}
    size = ["--frames", str(a.frames or 4096), "--warmup", str(a.warmup)]
    if a.part in ("old", "all") and a.parent_root:
        plib = ["--root", a.parent_root]
        run_one(["--one", "raw"] + size, a.limit)  # (discarded: the session's first process loads everything from a cold machine)
        for key, mode, what in (("old_paths_raw", "raw", "raw host frames"), ("old_paths_jpeg", "jpeg", "640x480 JPEG payloads"),
                                ("old_paths_dev", "dev", "device frames, 8 per call")):
            r = sides(out, key, "the queue with %s at 640x480: this commit against the parent; frames/s" % what,
                      ["--one", mode] + size, ["--one", mode] + size + plib, "parent", a.runs, a.limit)
            r["not_slower"] = r["median"]["this"] >= r["spread"]["parent"][0]
        out["condition_old_paths_not_slower"] = all(v["not_slower"] for k, v in out.items() if k.startswith("old_paths_"))
    if a.part in ("report", "all"):
        if not (a.part == "all" and a.parent_root):
            run_one(["--one", "raw"] + size, a.limit)  # (discarded)
        sides(out, "big_raw_vs_ceiling", "1280x960 raw host frames resized on the device (this) against the same queue fed 640x480 "
              "frames (the ceiling); frames/s", ["--one", "big_raw"] + size, ["--one", "raw"] + size, "ceiling_640x480", a.report_runs, a.limit)
        sides(out, "big_dev_vs_ceiling", "1280x960 device frames, 8 per call, resized on the device (this) against the same queue fed "
              "640x480 device frames (the ceiling); frames/s", ["--one", "big_dev"] + size, ["--one", "dev"] + size, "ceiling_640x480",
              a.report_runs, a.limit)
        host = ["--frames", str(a.frames or 1024), "--warmup", "128"]
        sides(out, "big_raw_vs_host_resize", "1280x960 raw host frames resized on the device (this) against cv::resize's scalar "
              "restatement on the caller's thread, then raw submit -- a LOWER BOUND for a host resize (no SIMD, one thread); frames/s",
              ["--one", "big_raw"] + host, ["--one", "host_resize"] + host, "host_resize_lower_bound", a.report_runs, a.limit)
    if a.kernel_stats:  # the profiler's *_kernel_stats.csv of a `--one big_dev` run of its own
        import csv
        for row in csv.DictReader(open(a.kernel_stats)):
            if "resize_gray_kernel" in row["Name"]:
                calls, avg = int(row["Calls"]), float(row["AverageNs"])
                # a launch takes a batch's run of frames: its bytes follow from the frames resized, not from the call count
                per_frame = 2 * (BW * BH + W * H)
                out["resize_kernel"] = {"what": "resize_gray_kernel over the batches of a `--one big_dev` run, from a profiler run of its "
                                                "own (kernel trace + stats, no counters); bytes = source + destination from the shapes; "
                                                "the share is the kernel's own, not the queue's",
                                        "calls": calls, "average_ns": avg, "min_ns": int(row["MinNs"]), "max_ns": int(row["MaxNs"]),
                                        "total_ns": int(row["TotalDurationNs"]), "bytes_per_stereo_frame": per_frame}
                # (the profiled run: the default --frames and --warmup of `--one big_dev`, every frame resized once)
                n = (a.frames or 4096) + a.warmup
                rate = n * per_frame / (int(row["TotalDurationNs"]) * 1e-9)
                out["resize_kernel"].update({"stereo_frames": n, "bytes_per_s": round(rate), "share_of_hbm_peak_8TBps": round(rate / HBM_PEAK, 4)})
    if a.bench_dir:  # this_*.json / parent_*.json: the last line of bench.py --gpus 1 --steps 20 --warmup 3, run alternating
        out["bench_py"] = {"what": "bench.py --gpus 1 --steps 20 --warmup 3, this commit and the parent alternating; stereo frames/s"}
        for side in ("this", "parent"):
            out["bench_py"][side] = [json.loads(f.read_text().strip().splitlines()[-1])["value"]
                                     for f in sorted(Path(a.bench_dir).glob(side + "_*.json"))]
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
