#!/usr/bin/env python3
"""What the debug images cost the queue: frames per second of ObserveOdometry + ObserveImage called from C++
(vsfh_time_sequence, as tools/time_frontend.py queued_fps) at 640x480 / 2000 features / depth 256 (128 per batch), with
FrontendConfig::debug_images_ off and on, and the device-to-host copy rate of one node's images (1280x480x3 + 640x480x3 =
2.76 MB) measured alone, which bounds the device's part of the debug mode (drawn in the batch's tail, copied into the pinned
debug ring).  Every image is kept, as the reference keeps them
(2.76 MB of host memory per node), so the runs are short.
    python tools/time_debug_images.py [--json] [n_frames]     (default 544: 512 steady frames)"""
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch  # (before libvsf_hip.so: the other order leaves torch without GPUs)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from vision_slam_frontend_amd import frontend, synth  # noqa: E402


def queued_fps(debug: bool, n_frames: int, nfeatures: int = 2000, depth: int = 256):
    sc = synth.Scene(640, 480)
    frames = np.stack([np.stack([sc.render(f, 0), sc.render(f, 1)]) for f in range(32)]).astype(np.uint8)
    F = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    fe = frontend.Frontend(640, 480, nfeatures=nfeatures, fundamental=F, debug_images=debug)
    fe.set_pipelined(True)
    fe.set_queue(depth, 0, 0)
    fps, mean_ms, _ = fe.time_sequence(frames, n_frames, warm=32)
    n_img = (frontend.lib().vsfh_num_debug_images(fe._h, 0), frontend.lib().vsfh_num_debug_images(fe._h, 1))
    fe.close()
    return fps, mean_ms, n_img


def copy_bound(reps: int = 200):
    """Frames per second that the pageable device-to-host copy of one node's two images alone allows."""
    d = torch.empty(480 * 1280 * 3 + 480 * 640 * 3, dtype=torch.uint8, device="cuda:0")
    h = np.empty(d.numel(), np.uint8)
    ht = torch.from_numpy(h)
    for _ in range(10):
        ht.copy_(d)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        ht.copy_(d)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    return 1.0 / dt, d.numel() / dt / 1e9


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--json"]
    n = int(args[0]) if args else 544
    rec = {}
    for debug in (False, True):
        fps, ms, n_img = queued_fps(debug, n)
        key = "debug_on" if debug else "debug_off"
        rec[key] = {"frames_per_s": fps, "observe_image_ms_mean": ms, "images": n_img}
        print("debug images %-3s %8.0f frames/s, %.3f ms inside ObserveImage (mean)%s" %
              ("on" if debug else "off", fps, ms, ", %d match / %d stereo images" % n_img if debug else ""))
    fps, gbs = copy_bound()
    rec["d2h_copy_bound"] = {"frames_per_s": fps, "GB_per_s": gbs}
    print("copy bound: one node's 2.76 MB device -> pageable host %.1f GB/s = %.0f frames/s" % (gbs, fps))
    if "--json" in sys.argv[1:]:
        print(json.dumps({"what": "queue with debug images, 640x480 / 2000 features / depth 256 (tools/time_debug_images.py)",
                          "results": rec}))
