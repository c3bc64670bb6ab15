#!/usr/bin/env python3
"""What the RViz visualization costs a caller that asks for it after EVERY node, as the reference's driver does
(slam_frontend_main.cc:319-325): frames per second of ObserveOdometry + ObserveImage (+ the visualization) called from C++
at 640x480 / 2000 features / queue depth 256 (128 per batch).

    a    pipelined, FrontendConfig::visualization_ on: Frontend::GetVisualization after every node (it does not flush; the cloud
         is made in the batches' tails and only appended on the host)
    b    synchronous, the visualization on the host as the reference's driver computes it: GetSLAMProblem (a copy of the whole
         problem) + AddFeaturePoints / AddPoseGraph over every node so far, after every node -- work that grows with the square
         of the run length, so the figure belongs to ITS run length (n_frames)
    off  pipelined, the switch off: vsfh_time_sequence, the loop tools/time_frontend.py times.  The one mode a checkout without
         the visualization can run too: run it from the parent commit's tree and from this one alternately for the comparison

a and b use a rectified rig that fits the synthetic scenes (f = 500 px, baseline 0.4 m), so that the cloud is not empty: under the
reference's hard-coded projections every point of these scenes lies behind the camera.

Serialising the two messages is left out by default (--publish N: after every N-th node): a Marker carries the WHOLE cloud, so
publishing after every node copies memory that grows with the square of the run length in any implementation.

    python tools/time_observe_visualization.py MODE [n_frames] [--publish N] [--json]
                                                                        (defaults: a 4128, b 1056, off 4128 frames; 32 warm-up)"""
import json
import sys
from pathlib import Path

import numpy as np
import torch  # noqa: F401  (before libvsf_hip.so: the other order leaves torch without GPUs)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from vision_slam_frontend_amd import frontend, synth  # noqa: E402

F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
P_LEFT = np.float32([[500, 0, 320, 0], [0, 500, 240, 0], [0, 0, 1, 0]])
P_RIGHT = np.float32([[500, 0, 320, -200], [0, 500, 240, 0], [0, 0, 1, 0]])
WARM = 32


def frames():
    sc = synth.Scene(640, 480)
    return np.stack([np.stack([sc.render(f, 0), sc.render(f, 1)]) for f in range(32)]).astype(np.uint8)


def run(mode: str, n_frames: int, publish_every: int = 0, nfeatures: int = 2000, depth: int = 256) -> dict:
    src = frames()
    if mode == "off":
        fe = frontend.Frontend(640, 480, nfeatures=nfeatures, fundamental=F_RECT)
        fe.set_pipelined(True)
        fe.set_queue(depth, 0, 0)
        fps, mean_ms, _ = fe.time_sequence(src, n_frames, warm=WARM)
        fe.close()
        return {"frames_per_s": fps, "observe_image_ms_mean": mean_ms, "n_frames": n_frames}
    fe = frontend.Frontend(640, 480, nfeatures=nfeatures, fundamental=F_RECT, visualization=(mode == "a"))
    fe.set_projections(P_LEFT, P_RIGHT)
    fe.set_pipelined(mode == "a")
    if mode == "a":
        fe.set_queue(depth, 0, 0)
    fps, points = fe.time_visualization(src, n_frames, warm=WARM, host=(mode == "b"), publish_every=publish_every)
    stats = fe.queue_stats()
    fe.close()
    return {"frames_per_s": fps, "cloud_points": points, "n_frames": n_frames, "batches": stats["batches"],
            "max_batch": stats["max_batch"], "world_points_commands": stats.get("world_points_commands", 0)}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--json"]
    publish = 0
    if "--publish" in args:
        i = args.index("--publish")
        publish = int(args[i + 1])
        del args[i:i + 2]
    mode = args[0] if args else "a"
    if mode not in ("a", "b", "off"):
        sys.exit(__doc__)
    n = int(args[1]) if len(args) > 1 else {"a": 4128, "b": 1056, "off": 4128}[mode]
    rec = run(mode, n, publish)
    if "--json" in sys.argv[1:]:
        print(json.dumps({"mode": mode, **rec}))
    else:
        print("mode %s: %.0f frames/s over %d frames %s" % (mode, rec["frames_per_s"], n - WARM,
                                                          {k: v for k, v in rec.items() if k not in ("frames_per_s", "n_frames")}))
