#!/usr/bin/env python3
"""What a detection mask (include/vsf.h "Detection masks") costs on this build, at 640x480 / 2000 features / 256 stereo frames:

  1. the batched composed step of bench.py (ShardedStereoFrontend.step: extraction, stereo matcher, tail) with a half-plane
     mask on both eyes (vsf_set_image_masks) against no mask: alternating runs, every run on a fresh context -- frames per
     second, and FAST's own duration from its stage timer in a few steps with the blur back in line, no cross-step pipelining
     and a host wait per step;
  2. the ObserveImage queue at depth 256 with stream masks (vsf_observe_set_stream_masks) against without: raw host frames
     submitted as fast as the queue takes them, collected in order;
  3. one vsf_mask_set (the pyramid build, host mask; blocking) and the bytes a slot holds.

Writes medians and ranges to profiles/mask/mask.json.

    python tools/time_mask.py [--steps 20] [--warmup 5] [--runs 4] [--batch 256] [--out profiles/mask/mask.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FAST = "fast_score_nms"  # vsf_stage_name of FAST's timer


def half_plane(w, h):
    m = np.zeros((h, w), np.uint8)
    m[:, : w // 2] = 255
    return m


def step_run(masked, args, torch, capi, frontend, vd, d_imgs):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    calib = frontend.default_calibration().set("fundamental", [0, 0, 0, 0, 0, -1, 0, 1, 0])
    B = args.batch
    with torch.cuda.stream(stream):
        ctx = capi.Context(capi.default_params(args.width, args.height, max_images=2 * B, nfeatures=args.nfeatures))
        sf = vd.ShardedStereoFrontend(ctx, B, args.width, args.height, calib, window=1, device=dev, stream=stream)
        try:
            sf.keep_outputs = False
            if masked:
                ctx.mask_set(0, half_plane(args.width, args.height))
                ctx.mask_set(1, half_plane(args.width, args.height))
                ctx.set_image_masks(0, 1)
            ctx.set_pipeline(True)
            torch.cuda.synchronize()
            tune = sf.tune(d_imgs, steps=16, warm=3)  # (bench.py's set-up: which FAST launch form this run's steps take)
            k = 0
            for _ in range(args.warmup):
                sf.step(d_imgs[k % len(d_imgs)])
                k += 1
            sf.drain()
            status = max(c.sync(allow_capacity=True) for c in sf.contexts())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                sf.step(d_imgs[k % len(d_imgs)])
                k += 1
            sf.drain()
            torch.cuda.synchronize()
            elapsed = time.perf_counter() - t0
            status = max([status] + [c.sync(allow_capacity=True) for c in sf.contexts()])
            # every stage by itself
            ctx.set_blur_overlap(False)
            ctx.set_pipeline(False)
            ctx.sync(allow_capacity=True)
            ctx.profile_enable(True)
            inline = 4
            for _ in range(inline):
                sf.step(d_imgs[k % len(d_imgs)])
                k += 1
                sf.drain()
                torch.cuda.synchronize()
            stages = ctx.profile_read(reset=True)
            ctx.profile_enable(False)
            return {"frames_per_s": B * args.steps / elapsed, "ms_per_step": 1e3 * elapsed / args.steps,
                    "fast_ms_per_step": stages[FAST][0] / inline, "fast_launches_per_step": stages[FAST][1] / inline,
                    "fast_resident": tune["fast_resident"], "status": int(status)}
        finally:
            sf.close()
            ctx.close()


def queue_run(masked, args, capi, frontend, frames):
    calib = frontend.default_calibration().set("fundamental", [0, 0, 0, 0, 0, -1, 0, 1, 0])
    depth, life = args.depth, 3
    ctx = capi.Context(capi.default_params(args.width, args.height, max_images=2 * min(depth, 128), nfeatures=args.nfeatures))
    try:
        ctx.observe_configure(depth, 0, 0)
        if masked:
            ctx.mask_set(0, half_plane(args.width, args.height))
            ctx.mask_set(1, half_plane(args.width, args.height))
            ctx.observe_set_stream_masks(0, 0, 1)

        def rounds(n):
            tickets = []
            for i in range(n):
                if len(tickets) == depth:
                    ctx.observe_collect_bytes(tickets.pop(0), life)
                left, right = frames[i % len(frames)]
                tickets.append(ctx.observe_submit(left, right, calib, best_percent=0.3, frame_life=life))
            for t in tickets:
                ctx.observe_collect_bytes(t, life)

        rounds(depth)  # warm-up: the queue is built, every kernel has run
        n = args.queue_frames
        t0 = time.perf_counter()
        rounds(n)
        elapsed = time.perf_counter() - t0
        return {"frames_per_s": n / elapsed, "batches": ctx.observe_stats()["batches"]}
    finally:
        ctx.close()


def mask_set_cost(args, capi):
    with capi.Context(capi.default_params(args.width, args.height, max_images=2, nfeatures=args.nfeatures)) as ctx:
        m = half_plane(args.width, args.height)
        ctx.mask_set(0, m)  # (the slot's allocation and the kernels' first launch)
        ms = []
        for _ in range(9):
            t0 = time.perf_counter()
            ctx.mask_set(0, m)
            ms.append(1e3 * (time.perf_counter() - t0))
        return {"mask_set_ms": summary([{"v": v} for v in ms], "v"), "slot_bytes": ctx.mask_slot_bytes(), "levels": ctx.nlevels}


def summary(runs, key):
    v = [r[key] for r in runs]
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--depth", type=int, default=256)
    ap.add_argument("--queue-frames", type=int, default=1024)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mask" / "mask.json"))
    args = ap.parse_args()
    import torch

    from vision_slam_frontend_amd import buildinfo, capi, frontend, synth
    from vision_slam_frontend_amd import distributed as vd
    if not torch.cuda.is_available():
        print("time_mask.py: no GPU visible", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    batch = synth.bench_batch(args.batch, args.width, args.height, seed=synth.BASE_SEED)
    d_img = torch.from_numpy(batch).to(dev)
    d_imgs = [d_img, torch.roll(d_img, shifts=(3, 11), dims=(2, 3)), torch.roll(d_img, shifts=(8, 29), dims=(2, 3))]
    host_frames = [(np.ascontiguousarray(batch[i, 0]), np.ascontiguousarray(batch[i, 1])) for i in range(min(len(batch), 32))]
    out = {"what": "%d stereo frames of %dx%d per step, %d features, %d timed steps after %d, %d alternating runs a side; the queue "
                   "at depth %d over %d frames; mask: the left half plane on both eyes"
                   % (args.batch, args.width, args.height, args.nfeatures, args.steps, args.warmup, args.runs, args.depth, args.queue_frames),
           "device": torch.cuda.get_device_name(0), "source_hash": buildinfo.kernel_source_hash()}
    steps = {"none": [], "masked": []}
    queue = {"none": [], "masked": []}
    for _ in range(args.runs):
        for name in ("none", "masked"):
            r = step_run(name == "masked", args, torch, capi, frontend, vd, d_imgs)
            steps[name].append(r)
            print("step %s: %.0f frames/s, %.3f ms per step, FAST alone %.3f ms per step in %g launches, FAST form %d, status %d"
                  % (name, r["frames_per_s"], r["ms_per_step"], r["fast_ms_per_step"], r["fast_launches_per_step"], r["fast_resident"],
                     r["status"]), flush=True)
    for _ in range(args.runs):
        for name in ("none", "masked"):
            r = queue_run(name == "masked", args, capi, frontend, host_frames)
            queue[name].append(r)
            print("queue %s: %.0f frames/s in %d batches" % (name, r["frames_per_s"], r["batches"]), flush=True)
    out["step"] = {name: {"frames_per_s": summary(rs, "frames_per_s"), "ms_per_step": summary(rs, "ms_per_step"),
                          "fast_ms_per_step": summary(rs, "fast_ms_per_step"), "fast_launches_per_step": rs[0]["fast_launches_per_step"],
                          "fast_resident": [r["fast_resident"] for r in rs], "status": max(r["status"] for r in rs)}
                   for name, rs in steps.items()}
    out["step"]["masked_over_none_frames_per_s"] = out["step"]["masked"]["frames_per_s"]["median"] / out["step"]["none"]["frames_per_s"]["median"]
    out["step"]["masked_over_none_fast_ms"] = out["step"]["masked"]["fast_ms_per_step"]["median"] / out["step"]["none"]["fast_ms_per_step"]["median"]
    out["queue"] = {name: {"frames_per_s": summary(rs, "frames_per_s")} for name, rs in queue.items()}
    out["queue"]["masked_over_none_frames_per_s"] = out["queue"]["masked"]["frames_per_s"]["median"] / out["queue"]["none"]["frames_per_s"]["median"]
    out["mask_set"] = mask_set_cost(args, capi)
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"step_masked_over_none": out["step"]["masked_over_none_frames_per_s"],
                      "fast_ms_masked_over_none": out["step"]["masked_over_none_fast_ms"],
                      "queue_masked_over_none": out["queue"]["masked_over_none_frames_per_s"],
                      "mask_set_ms": out["mask_set"]["mask_set_ms"]["median"], "slot_bytes": out["mask_set"]["slot_bytes"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
