#!/usr/bin/env python3
"""Time ``features.matching`` on a rendered rig and print one JSON line:
python tools/probe_matching.py [n_frames] [width] [height]

The rig: n frames (default 6 of 1280 x 720) on a jittered yaw sweep 30 degrees apart, rendered
from one textured equirectangular panorama (synth.render_rig).  Reported: the detector, knn,
pack and RANSAC kernel times of the kernel timing registry (summed ms, launches), the wall time
of ``matching`` after one warm-up call, the ratio-test survivors and RANSAC inliers per pair, and
the score kernel's lane-evaluations (hypothesis x correspondence) per second against the VALU
issue peak divided by its VALU instructions per evaluation (``valu_per_eval``, read from the
kernel's inner loop with tools/isa_stats.py)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pano360_amd import engine, features, synth  # noqa: E402

VALU_PEAK = 256 * 4 * 32 * 2.4e9      # lane-instructions/s: 256 CUs x 4 SIMD32 x 2.4 GHz
VALU_PER_EVAL = 206 / 8              # ransac_score_kernel's inner loop: 206 VALU per 8 correspondences

n = int(sys.argv[1]) if len(sys.argv) > 1 else 6
w = int(sys.argv[2]) if len(sys.argv) > 2 else 1280
h = int(sys.argv[3]) if len(sys.argv) > 3 else 720
pano = synth.make_frame(7, 4096, 2048, "B")
rots, intrs = synth.make_cameras(n, w, h, step_deg=30.0, jitter=0.01, seed=3)
eng = engine.engine()
frames = synth.render_rig(pano, rots, intrs, w, h, eng.device)
detect = features.sift_detector(eng)
features.matching(frames, detect)                         # warm-up: graphs, allocations
torch.cuda.synchronize()
eng.timing(True)
t0 = time.perf_counter()
kpts, matches = features.matching(frames, detect)
wall = (time.perf_counter() - t0) * 1e3
times = eng.kernel_times()
eng.timing(False)
# survivors per pair: the same pack step again, its device counts read back
dets = [detect(f) for f in frames]
pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
packed = features._Pairs([k for k in kpts], [d[1] for d in dets], pairs, eng)
survivors = packed.counts.cpu().numpy()
inliers = packed.n_inl.cpu().numpy()
evals = float(sum(int(c) for c in survivors if c >= features.N_MIN_MATCH)) * 2000
score_ms = times.get("ransac_score_kernel", (0.0, 0))[0]
pick = ("scale_step_kernel", "sift_extrema_kernel", "sift_orient_kernel", "sift_describe_kernel",
        "knn2_kernel", "match_pack_kernel", "ransac_score_kernel", "ransac_finish_kernel")
print(json.dumps({
    "frames": n, "width": w, "height": h,
    "keypoints": [len(k) for k in kpts],
    "kernel_ms": {k: [round(times[k][0], 4), times[k][1]] for k in pick if k in times},
    "matching_wall_ms": round(wall, 2),
    "survivors": {f"{i}-{j}": int(c) for (i, j), c in zip(pairs, survivors)},
    "inliers": {f"{i}-{j}": int(c) for (i, j), c in zip(pairs, inliers) if c},
    "score_lane_evals_per_s": evals / (score_ms * 1e-3) if score_ms else None,
    "score_evals_peak_per_s": VALU_PEAK / VALU_PER_EVAL,
    "valu_per_eval": VALU_PER_EVAL,
}))
