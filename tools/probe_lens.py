"""Time the lens correction (lens.undistort_device, one native call a batch) on the frame sets of
the bench: 32 frames of 3840 x 2160 and 8 frames of 1920 x 1080, for both models and both
interpolations.

Per item, median / min / max over --reps runs, in ms, from device events around the call (the
host's share of a call is inside: allocation of the outputs, the frame records and their upload;
the focal lengths are fitted once, outside the timed calls, and that host time is printed too).
Beside the times: the bytes a correction must move at the least - every pixel read once and
written once, 6 bytes a pixel (1.6 GB for 32 x 4K) -, that count over the HBM peak, and the share
of the peak the median amounts to.  The frames are noise (the taps' values do not change the
work); the calibrations are a barrel lens of a few percent (k1 = -0.25 at f = 0.8 w) and a
fisheye of f = w / 3.
Prints one JSON line per item.

    python tools/probe_lens.py [--reps 20] [--small]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from probe_view import HBM_PEAK, timed  # noqa: E402

SETS = {"32x4k": (32, 3840, 2160), "8x1080p": (8, 1920, 1080)}
SMALL = {"4x270p": (4, 480, 270)}


def models_for(w, h):
    from pano360_amd import lens
    return {"brown": lens.LensModel("brown", 0.8 * w, 0.8 * w, w / 2 + 3.3, h / 2 - 2.1,
                                    (-0.25, 0.05, 1e-3, -5e-4, 0.0), (w, h)),
            "fisheye": lens.LensModel("fisheye", w / 3, w / 3, w / 2 + 3.3, h / 2 - 2.1,
                                      (0.02, -0.003, 0.0, 0.0), (w, h))}


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--small", action="store_true", help="a small set (a rehearsal)")
    args = parser.parse_args()
    if args.reps < 1:
        parser.error("--reps is at least 1")

    import torch
    from pano360_amd import engine, lens
    eng = engine.engine()
    for name, (n, w, h) in (SMALL if args.small else SETS).items():
        gen = torch.Generator(device=eng.device).manual_seed(n)
        frames = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=eng.device, generator=gen)
                  for _ in range(n)]
        nbytes = 6 * n * w * h
        floor_ms = 1e3 * nbytes / HBM_PEAK
        for kind, model in models_for(w, h).items():
            t0 = time.perf_counter()
            focal = lens.fit_focal(model)
            fit_ms = 1e3 * (time.perf_counter() - t0)
            for interp in ("cubic", "linear"):
                stats, _ = timed(lambda: lens.undistort_device(frames, model, interp, focal, eng),
                                 args.reps)
                print(json.dumps({"item": f"{name}_{kind}_{interp}", "frames": [n, w, h],
                                  "focal": round(focal, 3), "fit_focal_host_ms": round(fit_ms, 2),
                                  "ms": stats, "bytes": nbytes, "hbm_floor_ms": round(floor_ms, 4),
                                  "share_of_hbm_peak": round(floor_ms / stats["median"], 4)}),
                      flush=True)
        del frames
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
