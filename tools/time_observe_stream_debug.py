#!/usr/bin/env python3
"""Debug images for every stream of the ObserveImage queue (vsf_observe_set_debug_seeds), measured at 640x480 / 2000
features / depth 256 (128 frames per batch).  Each run is one process; three runs a side, the sides alternating (and who goes first
alternating too), behind one discarded process that warms the machine.

  old paths   the queue with debug images off, with the old switch (raw canvases), with the old switch and JPEG files at
              quality 95: this library against --parent-root (a built checkout of the parent commit).  The condition: this
              commit's median is not below the parent's lowest run.
  report      one stream with a seed against the old switch, raw and JPEG; 8 and 32 streams with seeds and JPEG files in ONE
              queue against as many one-stream contexts with the old switch run one after the other; the submitting
              thread's time per frame in both modes (what the dropped rand() calls were worth).
  The colour kernel's own time comes from a profiler run of `--one seeded_raw` (a single-stream batch of 128 frames).

  python tools/time_observe_stream_debug.py [--parent-root DIR] [--part old|report|all]     then the JSON file
  python tools/time_observe_stream_debug.py --one MODE [--streams S] [--root DIR]             one run, one JSON line"""
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
W, H, NF, DEPTH, BATCH, LIFE = 640, 480, 2000, 256, 128, 5
MODES = ("off", "old_raw", "old_jpeg", "seeded_raw", "seeded_jpeg", "contexts_jpeg")


def one(a):
    import torch  # noqa: F401  (before libvsf_hip.so: the other order leaves torch without GPUs)

    if a.root:  # another checkout's package and library (the parent commit's, built there)
        sys.path.insert(0, str(Path(a.root).resolve()))
    else:
        sys.path.insert(0, str(ROOT))
    from vision_slam_frontend_amd import capi, frontend, synth
    assert Path(capi.__file__).resolve().is_relative_to(Path(a.root or ROOT).resolve())
    L = capi.lib()
    calib = frontend.default_calibration().set("fundamental", np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32))
    bp = float(np.float32(0.3))
    frames = synth.bench_batch(16, W, H)
    src = [(frames[i, 0].ctypes.data, frames[i, 1].ctypes.data) for i in range(len(frames))]
    S, mode = a.streams, a.one
    seeded, jpeg = mode.startswith("seeded"), mode.endswith("jpeg")
    ticket, view, nbytes = C.c_int64(), C.c_void_p(), C.c_size_t()

    def context(n_streams):
        ctx = capi.Context(capi.default_params(W, H, max_images=2 * BATCH, nfeatures=NF))
        ctx.observe_configure(DEPTH, 0, 0)
        if n_streams > 1:
            ctx.observe_set_streams(n_streams)
        if seeded:
            ctx.observe_set_debug_seeds(np.arange(1, n_streams + 1, dtype=np.uint32))
        if mode != "off":
            assert L.vsf_observe_set_debug_images(ctx._h, 1) == 0
        if jpeg:
            assert L.vsf_observe_set_debug_jpeg(ctx._h, 95) == 0
        return ctx

    def drive(ctx, n_streams, n_frames, warmup):
        """-> (seconds, seconds inside the submit calls) for n_frames frames, round-robin over the streams."""
        pending, t0, in_submit = [], None, 0.0

        def collect():
            assert L.vsf_observe_collect_view(ctx._h, pending.pop(0), C.byref(view), C.byref(nbytes)) == 0

        for g in range(warmup + n_frames):
            if g == warmup:  # the clock starts on an empty queue
                while pending:
                    collect()
                t0, in_submit = time.perf_counter(), 0.0
            while len(pending) >= DEPTH:
                collect()
            left, right = src[g % len(src)]
            h0 = time.perf_counter()
            if n_streams > 1:
                st = L.vsf_observe_submit_stream(ctx._h, g % n_streams, left, right, W, H, W, C.byref(calib), bp, LIFE, C.byref(ticket))
            else:
                st = L.vsf_observe_submit(ctx._h, left, right, W, H, W, C.byref(calib), bp, LIFE, C.byref(ticket))
            in_submit += time.perf_counter() - h0
            assert st == 0, st
            pending.append(ticket.value)
        while pending:
            collect()
        return time.perf_counter() - t0, in_submit

    if mode == "contexts_jpeg":  # S one-stream contexts with the old switch, one after the other: each takes its share
        per = a.frames // S
        dt = sub = 0.0
        for _ in range(S):
            with context(1) as ctx:
                d, s = drive(ctx, 1, per, min(a.warmup, per))
                dt, sub = dt + d, sub + s
        n = per * S
    else:
        with context(S) as ctx:
            dt, sub = drive(ctx, S, a.frames, a.warmup)
            stats = ctx.observe_stats()
        n = a.frames
        assert stats.get("seeded_colour_frames", 0) == ((a.frames + a.warmup) if seeded else 0)
    print(json.dumps({"mode": mode, "streams": S, "root": "parent" if a.root else "this", "frames": n,
                      "frames_per_s": round(n / dt, 1), "submit_us_per_frame": round(sub / n * 1e6, 2)}))


def run_one(args):
    p = subprocess.run([sys.executable, __file__] + args, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit("run %s failed (%d): %s" % (args, p.returncode, p.stderr[-2000:]))
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(rec), flush=True)
    return rec


def sides(out, key, what, this_args, other_args, other_name, runs=3):
    """`runs` runs a side, alternating; the medians, every run, and the other side's spread."""
    got = {"this": [], other_name: []}
    for i in range(runs):  # (who goes first alternates too: a run may inherit something from the process before it)
        for who in (("this", other_name) if i % 2 == 0 else (other_name, "this")):
            got[who].append(run_one(this_args if who == "this" else other_args))
    fps = {k: [r["frames_per_s"] for r in v] for k, v in got.items()}
    out[key] = {"what": what, "median": {k: statistics.median(v) for k, v in fps.items()},
                "spread_" + other_name: [min(fps[other_name]), max(fps[other_name])],
                "submit_us_per_frame_median": {k: statistics.median(r["submit_us_per_frame"] for r in v) for k, v in got.items()},
                "runs": got}
    return out[key]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", choices=MODES)
    ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--frames", type=int, default=0, help="timed frames of a run (0: 16384 with debug images off, 4096 for the other "
                    "old paths -- a third of a second and more --, 1024 for the report)")
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--root", default="", help="--one: another checkout (built) than this one to import the package from")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit")
    ap.add_argument("--part", choices=["old", "report", "all", "none"], default="all")
    ap.add_argument("--old-runs", type=int, default=0, help="runs a side of the old paths (0: --runs)")
    ap.add_argument("--kernel-stats", default="", help="a profiler's kernel_stats.csv to take the colour kernel's time from")
    ap.add_argument("--bench-dir", default="", help="a directory of bench.py result lines (this_*.json, parent_*.json) to record")
    ap.add_argument("--runs", type=int, default=3, help="runs a side")
    ap.add_argument("--old-modes", default="off,old_raw,old_jpeg", help="which of the old paths to measure")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r13" / "observe_stream_debug.json"))
    a = ap.parse_args()
    if a.one:
        a.frames = a.frames or 1024
        return one(a)
    out_path = Path(a.out)
    out = json.loads(out_path.read_text()) if out_path.exists() else {}
    size_of = lambda n: ["--frames", str(a.frames or n), "--warmup", str(a.warmup)]  # noqa: E731
    size = size_of(1024)
    if a.part in ("old", "all") and a.parent_root:
        plib = ["--root", a.parent_root]
        run_one(["--one", "off"] + size)  # (discarded: the session's first process loads everything from a cold machine)
        for key, mode, what in (("old_paths_off", "off", "debug images off"),
                                ("old_paths_raw", "old_raw", "the old switch, raw canvases"),
                                ("old_paths_jpeg", "old_jpeg", "the old switch, JPEG files at quality 95")):
            if mode not in a.old_modes.split(","):
                continue
            long = size_of(16384 if mode == "off" else 4096)
            r = sides(out, key, "the queue with %s: this commit against the parent; frames/s" % what,
                      ["--one", mode] + long, ["--one", mode] + long + plib, "parent", a.old_runs or a.runs)
            r["not_slower"] = r["median"]["this"] >= r["spread_parent"][0]
        out["condition_old_paths_not_slower"] = all(v["not_slower"] for k, v in out.items() if k.startswith("old_paths_"))
    if a.part in ("report", "all"):
        for form in ("raw", "jpeg"):
            sides(out, "one_stream_" + form, "one stream: a seed (this) against the old switch, %s; frames/s" % form,
                  ["--one", "seeded_" + form] + size, ["--one", "old_" + form] + size, "old_switch", a.runs)
        for S in (8, 32):
            sides(out, "streams_%d_jpeg" % S,
                  "%d streams with seeds and JPEG files in one queue (this) against %d one-stream contexts with the old switch "
                  "run one after the other; frames/s" % (S, S),
                  ["--one", "seeded_jpeg", "--streams", str(S)] + size, ["--one", "contexts_jpeg", "--streams", str(S)] + size,
                  "contexts_in_turn", a.runs)
    if a.kernel_stats:  # the profiler's *_kernel_stats.csv of a `--one seeded_raw` run of its own
        import csv
        for row in csv.DictReader(open(a.kernel_stats)):
            if "debug_colours_kernel" in row["Name"]:
                out["colour_kernel"] = {"what": "debug_colours_kernel over single-stream batches of 128 frames, from a profiler run of "
                                                "`--one seeded_raw` of its own (kernel trace + stats)",
                                        "calls": int(row["Calls"]), "average_ns": float(row["AverageNs"]), "min_ns": int(row["MinNs"]),
                                        "max_ns": int(row["MaxNs"]), "share_of_kernel_time_percent": float(row["Percentage"])}
    if a.bench_dir:  # this_*.json / parent_*.json: the last line of bench.py --gpus 1 --steps 20 --warmup 3, run alternating
        out["bench_py"] = {"what": "bench.py --gpus 1 --steps 20 --warmup 3, this commit and the parent alternating; stereo frames/s"}
        for side in ("this", "parent"):
            out["bench_py"][side] = [json.loads(f.read_text())["value"] for f in sorted(Path(a.bench_dir).glob(side + "_*.json"))]
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
