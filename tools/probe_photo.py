"""Time the photometric alignment (photo.estimate_device: three passes of one native statistics
call and one host solve each; photo.apply_device: one native call) on the rigs of the bench: 32
frames of 3840 x 2160 (a 155 degree sweep) and 8 frames of 1920 x 1080 (140 degrees).

Per item, median / min / max over --reps runs, in ms, from device events around the call (the
host's share of a call is inside: the pair table, the records and their upload, the download of
the sums and the solves; the frames are on the device before).  The statistics kernel is also
timed on its own (the library's per-kernel events, one pass).  Beside the times, the bytes each
must move at the least and that count over the HBM peak:
  a statistics pass  15 bytes per sample - the pixel of frame i and the four taps of frame j -,
                     the samples counted by the pass itself (every weight 1); neighbouring
                     samples share no byte once the lattice step is 2 or more
  the correction     every pixel read once and written once, 6 bytes a pixel
The frames are noise in 64 .. 191: every sample passes the range test, which is the most work a
rig of that geometry can ask for (the values do not change the work otherwise).  The fitted
parameters of such frames mean nothing; the correction is timed with gains of +-20 % and the
falloff a = (-0.45, 0.10).  Prints one JSON line per item.

    python tools/probe_photo.py [--reps 10] [--small]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from probe_view import HBM_PEAK, timed  # noqa: E402

SETS = {"32x4k": (32, 3840, 2160, 155.0), "8x1080p": (8, 1920, 1080, 140.0)}
SMALL = {"4x270p": (4, 480, 270, 70.0)}


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--small", action="store_true", help="a small set (a rehearsal)")
    args = parser.parse_args()
    if args.reps < 1:
        parser.error("--reps is at least 1")

    import torch
    from pano360_amd import engine, photo, synth
    eng = engine.engine()
    for name, (n, w, h, sweep) in (SMALL if args.small else SETS).items():
        gen = torch.Generator(device=eng.device).manual_seed(n)
        frames = [torch.randint(64, 192, (h, w, 3), dtype=torch.uint8, device=eng.device, generator=gen)
                  for _ in range(n)]
        rots, intrs = synth.make_cameras(n, w, h, sweep_deg=sweep)
        step = photo.default_step([(h, w)])
        pairs = photo.pair_table([(h, w)] * n, rots, intrs)

        # one pass on its own: the samples it takes, the kernel's own time
        eng.timing(True)
        _, sums = photo.stats_device(frames, rots, intrs, step=step, eng=eng, pairs=pairs)
        kernel_ms = eng.kernel_times().get("photo_stats_kernel", (0.0, 0))[0]
        eng.timing(False)
        samples = int(sums[:, 0].sum())
        pass_bytes = 15 * samples
        stats, _ = timed(lambda: photo.stats_device(frames, rots, intrs, step=step, eng=eng, pairs=pairs),
                         args.reps)
        print(json.dumps({"item": f"{name}_stats_pass", "frames": [n, w, h], "step": step,
                          "pairs": len(pairs), "pairs_with_samples": int((sums[:, 0] > 0).sum()),
                          "samples": samples, "ms": stats, "kernel_ms": round(kernel_ms, 4),
                          "bytes": pass_bytes,
                          "hbm_floor_ms": round(1e3 * pass_bytes / HBM_PEAK, 5)}), flush=True)
        stats, model = timed(lambda: photo.estimate_device(frames, rots, intrs, eng=eng), args.reps)
        print(json.dumps({"item": f"{name}_estimate", "frames": [n, w, h], "step": step,
                          "passes": photo.ROUNDS + 1, "ms": stats, "bytes": 3 * pass_bytes,
                          "hbm_floor_ms": round(3e3 * pass_bytes / HBM_PEAK, 5)}), flush=True)

        rng = np.random.default_rng(n)
        model = photo.PhotoModel(np.log(rng.uniform(0.8, 1.2, size=(n, 3))), (-0.45, 0.10, 0.0))
        nbytes = 6 * n * w * h
        floor_ms = 1e3 * nbytes / HBM_PEAK
        stats, _ = timed(lambda: photo.apply_device(frames, model, eng), args.reps)
        print(json.dumps({"item": f"{name}_apply", "frames": [n, w, h], "ms": stats, "bytes": nbytes,
                          "hbm_floor_ms": round(floor_ms, 4),
                          "share_of_hbm_peak": round(floor_ms / stats["median"], 4)}), flush=True)
        del frames
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
