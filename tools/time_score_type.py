#!/usr/bin/env python3
"""What cv::ORB::FAST_SCORE (vsf_params::score_type 1) buys against HARRIS_SCORE on this build: the batched composed step of
bench.py (ShardedStereoFrontend.step: extraction, stereo matcher, tail) on 256 stereo frames of 640x480 per step, at 2000 and
at 10 000 features.  Four runs a side, alternating (HARRIS, FAST_SCORE, HARRIS, ...), every run on a fresh context: warm-up
steps, timed steps, then a few steps with the blur back in line, no cross-step pipelining and a host wait per step, whose
stage timers give the selection's OWN duration (beside the blur its timer is a wall span on a shared chip).

Writes medians and ranges to profiles/score_type/score_type.json.

    python tools/time_score_type.py [--steps 20] [--warmup 5] [--runs 4] [--batch 256] [--out profiles/score_type/score_type.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SELECT = "select_harris_angle"  # vsf_stage_name of the selection's timer, in either mode


def one_run(score_type, nfeatures, args, torch, capi, frontend, synth, vd, d_imgs):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    calib = frontend.default_calibration().set("fundamental", [0, 0, 0, 0, 0, -1, 0, 1, 0])
    B = args.batch
    with torch.cuda.stream(stream):
        ctx = capi.Context(capi.default_params(args.width, args.height, max_images=2 * B, nfeatures=nfeatures, score_type=score_type))
        sf = vd.ShardedStereoFrontend(ctx, B, args.width, args.height, calib, window=1, device=dev, stream=stream,
                                      match_on_tail=nfeatures >= 5000)
        try:
            sf.keep_outputs = False
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
                    "select_ms_per_step": stages[SELECT][0] / inline, "select_launches_per_step": stages[SELECT][1] / inline,
                    "fast_resident": tune["fast_resident"], "status": int(status)}
        finally:
            sf.close()
            ctx.close()


def summary(runs, key):
    v = [r[key] for r in runs]
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--nfeatures", type=int, nargs="*", default=[2000, 10000])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "score_type" / "score_type.json"))
    args = ap.parse_args()
    import torch

    from vision_slam_frontend_amd import buildinfo, capi, frontend, synth
    from vision_slam_frontend_amd import distributed as vd
    if not torch.cuda.is_available():
        print("time_score_type.py: no GPU visible", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    frames = synth.bench_batch(args.batch, args.width, args.height, seed=synth.BASE_SEED)
    d_img = torch.from_numpy(frames).to(dev)
    d_imgs = [d_img, torch.roll(d_img, shifts=(3, 11), dims=(2, 3)), torch.roll(d_img, shifts=(8, 29), dims=(2, 3))]
    out = {"what": "batched composed step, %d stereo frames of %dx%d per step, %d timed steps after %d, %d alternating runs a side"
                   % (args.batch, args.width, args.height, args.steps, args.warmup, args.runs),
           "device": torch.cuda.get_device_name(0), "source_hash": buildinfo.kernel_source_hash(), "configs": {}}
    for nf in args.nfeatures:
        runs = {"harris": [], "fast_score": []}
        for _ in range(args.runs):
            for name, st in (("harris", capi.HARRIS_SCORE), ("fast_score", capi.FAST_SCORE)):
                r = one_run(st, nf, args, torch, capi, frontend, synth, vd, d_imgs)
                runs[name].append(r)
                print("nfeatures %d %s: %.0f frames/s, %.3f ms per step, selection alone %.3f ms per step, FAST form %d, status %d"
                      % (nf, name, r["frames_per_s"], r["ms_per_step"], r["select_ms_per_step"], r["fast_resident"], r["status"]), flush=True)
        rec = {}
        for name, rs in runs.items():
            rec[name] = {"frames_per_s": summary(rs, "frames_per_s"), "ms_per_step": summary(rs, "ms_per_step"),
                         "select_ms_per_step": summary(rs, "select_ms_per_step"),
                         "select_launches_per_step": rs[0]["select_launches_per_step"],
                         "fast_resident": [r["fast_resident"] for r in rs], "status": max(r["status"] for r in rs)}
        rec["fast_score_over_harris_frames_per_s"] = rec["fast_score"]["frames_per_s"]["median"] / rec["harris"]["frames_per_s"]["median"]
        rec["select_ms_saved_per_step"] = rec["harris"]["select_ms_per_step"]["median"] - rec["fast_score"]["select_ms_per_step"]["median"]
        out["configs"]["nfeatures_%d" % nf] = rec
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: {"fast_score_over_harris": v["fast_score_over_harris_frames_per_s"],
                          "select_ms_saved_per_step": v["select_ms_saved_per_step"]} for k, v in out["configs"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
