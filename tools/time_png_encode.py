#!/usr/bin/env python3
"""Throughput of the PNG encoder: N images of 640x480 per vsf_png_encode_batch_dev call (device to device), gray and BGR, against
the same images through the system's libpng on ONE host core (tests/png_enc_ref.py: the library driven as cv::imencode(".png")
drives it); then the ObserveImage queue at 640x480 / 2000 features / depth 256 (as tools/time_debug_images.py runs it) with the
debug images leaving as raw canvases, as JPEG files of quality 95 and as PNG files, in three alternating runs on the same box,
with the bytes that go home per frame.  Every measurement is a child process of its own under its own time limit; the first
that fails stops the rest.  Writes one JSON object; with a path argument, into that file too.
    python tools/time_png_encode.py [n_images] [out.json] [--no-queue]"""
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

W, H, REPS = 640, 480, 5


def encode_case(ch: int, n: int) -> dict:
    import numpy as np
    import torch

    import png_enc_ref as ref
    from vision_slam_frontend_amd import capi, synth
    dev = torch.device("cuda", 0)
    gray = synth.bench_batch(8, W, H, n_scenes=4).reshape(-1, H, W)
    base = gray if ch == 1 else np.stack([gray, np.roll(gray, 5, 1), np.roll(gray, 3, 2)], -1)
    imgs = np.ascontiguousarray(np.stack([base[i % len(base)] for i in range(n)]))
    stride = capi.png_encode_capacity(W, H, ch)
    with capi.Context(capi.default_params(W, H, max_images=2, nfeatures=100)) as ctx:
        d_src = torch.from_numpy(imgs).to(dev)
        d_out = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        run = lambda: ctx.png_encode_batch_dev(d_src.data_ptr(), n, W, H, ch, W * H * ch, W * ch, d_out.data_ptr(), stride,  # noqa: E731
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
    n_host = min(n, 32)
    host_files = [ref.imencode(imgs[i]) for i in range(n_host)]
    host = (time.perf_counter() - t0) / n_host
    assert first == host_files[0], "the device's file differs from libpng's"
    dt = float(np.median(times))
    return {"channels": ch, "mean_file_bytes": float(sizes.mean()), "raw_bytes": W * H * ch,
            "file_over_raw": float(sizes.mean()) / (W * H * ch), "ms_per_call_median": dt * 1e3,
            "ms_per_call_all": [t * 1e3 for t in times], "images_per_s": n / dt, "libpng_one_core_images_per_s": 1.0 / host}


def queue_case(form: str, n_frames: int = 544, nfeatures: int = 2000, depth: int = 256) -> dict:
    """tools/time_debug_images.py queued_fps with the debug images on: raw, JPEG files or PNG files."""
    import numpy as np

    from vision_slam_frontend_amd import frontend, synth
    sc = synth.Scene(640, 480)
    frames = np.stack([np.stack([sc.render(f, 0), sc.render(f, 1)]) for f in range(32)]).astype(np.uint8)
    F = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    fe = frontend.Frontend(640, 480, nfeatures=nfeatures, fundamental=F, debug_images=True,
                           debug_jpeg_quality=95 if form == "jpeg" else 0, debug_png=form == "png")
    fe.set_pipelined(True)
    fe.set_queue(depth, 0, 0)
    fps, mean_ms, _ = fe.time_sequence(frames, n_frames, warm=32)
    size = len(fe.last_debug_image_compressed(stereo=True) or b"") + len(fe.last_debug_image_compressed() or b"")
    fe.close()
    return {"frames_per_s": fps, "bytes_home": size if form != "raw" else 9 * 640 * 480}


def child(args, limit):
    p = subprocess.run([sys.executable, __file__, "--child"] + [str(a) for a in args], capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("measurement %s failed (%d): the rest is not run" % (args, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    if "--child" in sys.argv:
        a = sys.argv[sys.argv.index("--child") + 1:]
        print(json.dumps(encode_case(int(a[1]), int(a[2])) if a[0] == "encode" else queue_case(a[1])))
        raise SystemExit(0)
    ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
    N = int(ARGS[0]) if ARGS else 512
    result = {"what": "vsf_png_encode_batch_dev alone, %d images of %dx%d per call" % (N, W, H), "cases": []}
    for ch in (1, 3):
        c = child(["encode", ch, N], 300)
        result["cases"].append(c)
        print("%d channel(s): %d images in %.2f ms = %.0f images/s (files of %.0f KB for %.0f KB raw); libpng on one core %.0f images/s"
              % (ch, N, c["ms_per_call_median"], c["images_per_s"], c["mean_file_bytes"] / 1024, c["raw_bytes"] / 1024,
                 c["libpng_one_core_images_per_s"]), flush=True)
    if "--no-queue" not in sys.argv[1:]:
        keys = {"raw": "raw_canvases", "jpeg": "jpeg_files_q95", "png": "png_files"}
        runs = {k: [] for k in keys.values()}
        home = {}
        for rep in range(3):  # alternating, so that a drift of the box shows in all three
            for form, key in keys.items():
                c = child(["queue", form], 300)
                runs[key].append(c["frames_per_s"])
                home[key] = max(home.get(key, 0), c["bytes_home"])
                print("queue, debug images as %-14s run %d: %8.0f frames/s" % (key, rep, c["frames_per_s"]), flush=True)
        med = {k: sorted(v)[1] for k, v in runs.items()}
        result["queue"] = {"what": "ObserveImage queue, 640x480 / 2000 features / depth 256, debug images on; frames/s of alternating runs",
                           "frames_per_s": runs, "median": med, "bytes_home_per_frame": home,
                           "png_beats_raw_canvases": med["png_files"] > med["raw_canvases"]}
    print(json.dumps(result))
    if len(ARGS) > 1:
        Path(ARGS[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(ARGS[1]).write_text(json.dumps(result, indent=1) + "\n")
