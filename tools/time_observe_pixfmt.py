#!/usr/bin/env python3
"""Raw frames of other pixel formats than mono8 in the ObserveImage queue (vsf_observe_submit_stream_pix, vsf_observe_submit_dev
with a VSF_PIX_* code), measured with a 640x480 context / 2000 features / depth 256 (128 frames per batch).  Each run is one
process under its own time limit; the sides alternate (and who goes first alternates too), behind one discarded process that
warms the machine.

  old paths   the raw queue, the compressed queue (640x480 JPEG) and the device queue (8 frames per call), and the Bayer
              kernel on 512 RGGB mosaics of 640x480: this library against --parent-root (a built checkout of the parent
              commit), four runs a side.  The conditions: a queue's median is not below the parent's LOWEST run; the
              kernel's median time is not above the parent's SLOWEST run.
  report      raw host BGR8, raw host GRBG and device BGRA8 (8 per call) frames -- each against (a) the same queue fed the
              pre-converted gray frames, the ceiling, and (b) the conversion on the caller's thread (the oracle's scalar
              demosaic; for colour the numpy expression of RGB2Gray), then raw submit: a LOWER BOUND for a host converter.
  kernels     vsf_to_gray_batch_dev alone on 256 images (128 stereo frames) of 640x480, the host's clock around 20 back-to-back
              launches and one sync: microseconds per launch and source + destination bytes over that time as a share of the
              8 TB/s HBM peak (repeated launches over the same images: the Infinity Cache holds part of them).

  python tools/time_observe_pixfmt.py [--parent-root DIR] [--part old|report|kernels|all]     then the JSON file
  python tools/time_observe_pixfmt.py --one MODE [--root DIR]                                  one run, one JSON line"""
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
W, H, NF, DEPTH, BATCH, LIFE, PER_CALL = 640, 480, 2000, 256, 128, 5, 8
PIX = {"mono8": 0, "rggb": 1, "grbg": 16, "gbrg": 17, "bggr": 18, "bgr8": 19, "rgb8": 20, "bgra8": 21, "rgba8": 22}
BPP = {0: 1, 1: 1, 16: 1, 17: 1, 18: 1, 19: 3, 20: 3, 21: 4, 22: 4}
# queue modes: (pixel format, where the frames are, who converts)
QUEUE = {"raw": ("mono8", "host", None), "jpeg": ("mono8", "jpeg", None), "dev": ("mono8", "dev", None),
         "bgr_host": ("bgr8", "host", "gpu"), "grbg_host": ("grbg", "host", "gpu"), "bgra_dev": ("bgra8", "dev", "gpu"),
         "bgr_host_convert": ("bgr8", "host", "cpu"), "grbg_host_convert": ("grbg", "host", "cpu"),
         "bgra_host_convert": ("bgra8", "host", "cpu")}
MODES = tuple(QUEUE) + ("kernels", "bayer512")
HBM_PEAK = 8.0e12


def _colour(gray, bpp, rng):
    c = np.clip(gray[..., None].astype(np.int32) + rng.integers(-24, 25, gray.shape + (bpp,)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(c)


def _cpu_gray(img, pixfmt):
    if BPP[pixfmt] == 1:
        sys.path.insert(0, str(ROOT / "tests"))
        import pixfmt_ref
        return pixfmt_ref.to_gray(img, pixfmt)
    c = img.astype(np.uint32)
    b, r = (c[..., 2], c[..., 0]) if pixfmt in (20, 22) else (c[..., 0], c[..., 2])
    return ((1868 * b + 9617 * c[..., 1] + 4899 * r + 8192) >> 14).astype(np.uint8)


def kernels(a, capi, torch):
    """`reps` groups of 20 back-to-back launches on the context's stream, each group timed by the host's clock up to its sync."""
    out = {}
    ctx = capi.Context(capi.default_params(W, H, max_images=2, nfeatures=100))
    n = 512 if a.one == "bayer512" else 2 * BATCH
    fmts = ["rggb"] if a.one == "bayer512" else ["bgr8", "bgra8", "grbg", "rggb", "mono8"]
    for name in fmts:
        f, bpp = PIX[name], BPP[PIX[name]]
        src = torch.randint(0, 256, (n, H, W * bpp), dtype=torch.uint8, device="cuda:0")
        dst = torch.zeros((n, H, W), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

        def launch():
            if a.one == "bayer512":  # (the call the parent has too)
                ctx.bayer_bg_to_gray_batch_dev(src.data_ptr(), n, W, H, W * H, W, dst.data_ptr(), W * H, W)
            else:
                assert ctx.to_gray_batch_dev(src.data_ptr(), n, W, H, f, W * bpp * H, W * bpp, dst.data_ptr(), W * H, W) == 0
        for _ in range(5):
            launch()
        assert ctx.sync() == 0
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(20):
                launch()
            assert ctx.sync() == 0
            times.append((time.perf_counter() - t0) / 20)
        us = statistics.median(times) * 1e6
        nbytes = n * W * H * (bpp + 1)
        out[name] = {"images": n, "us_per_launch": round(us, 1), "us_min_max": [round(min(times) * 1e6, 1), round(max(times) * 1e6, 1)],
                     "bytes": nbytes, "share_of_hbm_peak_8TBps": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}
    ctx.close()
    print(json.dumps({"mode": a.one, "root": "parent" if a.root else "this", "timing": "host clock around 20 back-to-back launches "
                      "and one sync, median of %d" % a.reps, "kernels": out,
                      "us_per_launch": out["rggb"]["us_per_launch"]}))


def one(a):
    import torch  # (before libvsf_hip.so: the other order leaves torch without GPUs)

    sys.path.insert(0, str(Path(a.root).resolve()) if a.root else str(ROOT))
    from vision_slam_frontend_amd import capi, frontend, synth
    assert Path(capi.__file__).resolve().is_relative_to(Path(a.root or ROOT).resolve())
    if a.one in ("kernels", "bayer512"):
        return kernels(a, capi, torch)
    L = capi.lib()
    calib = frontend.default_calibration().set("fundamental", np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32))
    bp = float(np.float32(0.3))
    name, where, who = QUEUE[a.one]
    pixfmt, bpp = PIX[name], BPP[PIX[name]]
    gray = synth.bench_batch(16, W, H)
    rng = np.random.default_rng(1)
    frames = gray if bpp == 1 else np.stack([np.stack([_colour(gray[i, s], bpp, rng) for s in range(2)]) for i in range(len(gray))])
    ticket, view, nbytes = C.c_int64(), C.c_void_p(), C.c_size_t()
    files = dev = None
    if where == "jpeg":
        from PIL import Image

        def enc(img):
            b = io.BytesIO()
            Image.fromarray(img, "L").save(b, "JPEG", quality=90)
            return np.frombuffer(b.getvalue(), np.uint8)
        files = [(enc(frames[i, 0]), enc(frames[i, 1])) for i in range(len(frames))]
    if where == "dev":
        dev = torch.from_numpy(frames).to("cuda:0")
        torch.cuda.synchronize()
        arr = (capi.VsfDevFrame * PER_CALL)()
        tickets = (C.c_int64 * PER_CALL)()
        stream = torch.cuda.current_stream(0).cuda_stream
    if who == "cpu":
        _cpu_gray(frames[0, 0], pixfmt)  # (loads the oracle before the clock starts)
    ctx = capi.Context(capi.default_params(W, H, max_images=2 * BATCH, nfeatures=NF))
    ctx.observe_configure(DEPTH, 0, 0)
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
                arr[k] = capi.VsfDevFrame(l.data_ptr(), r.data_ptr(), W * bpp, W * bpp)
            st = L.vsf_observe_submit_dev(ctx._h, 0, arr, PER_CALL, pixfmt, C.c_void_p(stream or None), C.byref(calib), bp, LIFE, tickets)
            new = list(tickets)
        elif files is not None:
            l, r = files[i]
            st = L.vsf_observe_submit_compressed(ctx._h, l.ctypes.data, len(l), r.ctypes.data, len(r), 0, C.byref(calib), bp, LIFE,
                                                 C.byref(ticket))
            new = [ticket.value]
        else:
            l, r = frames[i, 0], frames[i, 1]
            if who == "cpu":  # (b): the conversion on the caller's thread, then a frame like any other
                l, r = _cpu_gray(l, pixfmt), _cpu_gray(r, pixfmt)
            if who == "gpu":
                st = L.vsf_observe_submit_stream_pix(ctx._h, 0, l.ctypes.data, r.ctypes.data, W, H, W * bpp, pixfmt, C.byref(calib), bp,
                                                     LIFE, C.byref(ticket))
            else:
                st = L.vsf_observe_submit(ctx._h, l.ctypes.data, r.ctypes.data, W, H, W, C.byref(calib), bp, LIFE, C.byref(ticket))
            new = [ticket.value]
        in_submit += time.perf_counter() - h0
        assert st == 0, st
        pending += new
    while pending:
        collect()
    dt = time.perf_counter() - t0
    stats = ctx.observe_stats()
    ctx.close()
    assert stats.get("pixfmt_frames", 0) == ((a.frames + a.warmup) if who == "gpu" else 0), stats
    print(json.dumps({"mode": a.one, "root": "parent" if a.root else "this", "frames": a.frames, "frames_per_s": round(a.frames / dt, 1),
                      "submit_us_per_frame": round(in_submit / a.frames * 1e6, 2)}))


def run_one(args, limit):
    p = subprocess.run([sys.executable, __file__] + args, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        raise SystemExit("run %s failed (%d): %s" % (args, p.returncode, p.stderr[-2000:]))
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(rec), flush=True)
    return rec


def sides(out, key, what, this_args, other_args, other_name, runs, limit, field="frames_per_s", other_first=False):
    """`runs` runs a side, alternating; the medians, every run, and both sides' spreads."""
    got = {"this": [], other_name: []}
    for i in range(runs):  # (who goes first alternates too: a run may inherit something from the process before it)
        for who in (("this", other_name) if (i + other_first) % 2 == 0 else (other_name, "this")):
            got[who].append(run_one(this_args if who == "this" else other_args, limit))
    val = {k: [r[field] for r in v] for k, v in got.items()}
    out[key] = {"what": what, "median": {k: statistics.median(v) for k, v in val.items()},
                "spread": {k: [min(v), max(v)] for k, v in val.items()}, "runs": got}
    return out[key]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--one", choices=MODES)
    ap.add_argument("--frames", type=int, default=0, help="timed frames of a run (0: 4096; 512 for the host conversions)")
    ap.add_argument("--warmup", type=int, default=256)
    ap.add_argument("--reps", type=int, default=15, help="kernels: timed groups of 20 launches")
    ap.add_argument("--root", default="", help="--one: another checkout (built) than this one to import the package from")
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit")
    ap.add_argument("--part", choices=["old", "report", "kernels", "all"], default="all")
    ap.add_argument("--runs", type=int, default=4, help="runs a side of the old paths")
    ap.add_argument("--report-runs", type=int, default=3, help="runs a side of the report")
    ap.add_argument("--parent-first", action="store_true", help="old paths: the parent takes the first run of the first pair")
    ap.add_argument("--limit", type=int, default=240, help="seconds a run may take")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r15" / "observe_pixfmt.json"))
    a = ap.parse_args()
    if a.one:
        a.frames = a.frames or (512 if a.one.endswith("_convert") else 4096)
        return one(a)
    out_path = Path(a.out)
    out = json.loads(out_path.read_text()) if out_path.exists() else {}
    size = ["--frames", str(a.frames or 4096), "--warmup", str(a.warmup)]
    run_one(["--one", "raw"] + size, a.limit)  # (discarded: the session's first process loads everything from a cold machine)
    if a.part in ("old", "all") and a.parent_root:
        plib = ["--root", a.parent_root]
        r = sides(out, "bayer_kernel_rggb_512", "the Bayer kernel on 512 RGGB mosaics of 640x480 (vsf_bayer_bg_to_gray_batch_dev): this "
                  "commit's generalised kernel against the parent's; microseconds per launch", ["--one", "bayer512"],
                  ["--one", "bayer512"] + plib, "parent", a.runs, a.limit, field="us_per_launch", other_first=a.parent_first)
        r["not_slower"] = r["median"]["this"] <= r["spread"]["parent"][1]
        for key, mode, what in (("old_paths_raw", "raw", "raw host frames"), ("old_paths_jpeg", "jpeg", "640x480 JPEG payloads"),
                                ("old_paths_dev", "dev", "device mono frames, 8 per call")):
            r = sides(out, key, "the queue with %s at 640x480: this commit against the parent; frames/s" % what,
                      ["--one", mode] + size, ["--one", mode] + size + plib, "parent", a.runs, a.limit, other_first=a.parent_first)
            r["not_slower"] = r["median"]["this"] >= r["spread"]["parent"][0]
        out["condition_old_paths_not_slower"] = all(v["not_slower"] for k, v in out.items() if k.startswith("old_paths_"))
    if a.part in ("report", "all"):
        host = ["--frames", str(a.frames or 512), "--warmup", "64"]
        for mode, ceiling, convert, what in (("bgr_host", "raw", "bgr_host_convert", "raw host BGR8 frames"),
                                             ("grbg_host", "raw", "grbg_host_convert", "raw host GRBG mosaics"),
                                             ("bgra_dev", "dev", "bgra_host_convert", "device BGRA8 frames, 8 per call")):
            sides(out, mode + "_vs_gray", "%s converted on the device (this) against the same queue fed pre-converted gray frames (the "
                  "ceiling); frames/s" % what, ["--one", mode] + size, ["--one", ceiling] + size, "gray_ceiling", a.report_runs, a.limit)
            sides(out, mode + "_vs_host_convert", "%s converted on the device (this) against the conversion on the caller's thread, then "
                  "raw submit -- a LOWER BOUND for a host converter (one thread, no SIMD of its own); frames/s" % what,
                  ["--one", mode] + host, ["--one", convert] + host, "host_convert_lower_bound", 2, a.limit)
    if a.part in ("kernels", "all"):
        out["kernels_128_stereo_frames"] = run_one(["--one", "kernels", "--reps", str(a.reps)], a.limit)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
