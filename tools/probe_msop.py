"""Time the MSOP detector per stage on the GPU, beside the reference's ``msop_detect`` on the CPU.

GPU: ``features.msop_detect_device`` on a seeded smoothed-noise frame of 1080 x 1920 and of
2160 x 3840 with the default ``max_feat``; per size the median wall time of whole calls (nothing
waited for inside) and, from separate calls in which every entry point is waited for, the median
seconds per stage (the kernels' time; the host's work between the calls is in the whole only).  CPU (with --reference DIR, on a machine that has the reference): the reference's
``msop_detect`` on the same frames through the NumPy stand-ins of tools/gen_msop_golden.py, one
run per size.  That is the comparison time; it measures the reference's algorithm in NumPy, not
OpenCV's speed.  Prints one JSON line.

    python tools/probe_msop.py [--reference DIR] [--no-gpu] [--repeats N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1080, 1920), (2160, 3840))


def frame_of(h, w):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import msop_model as mm
    return np.repeat(mm.smooth_noise(h, w, 41)[..., None], 3, axis=2)


STAGES = {"pano_gray_u8": "gray_pyrdown", "pano_pyr_down": "gray_pyrdown", "pano_harris": "harris",
          "pano_msop_candidates": "candidates_cut", "pano_msop_cut": "candidates_cut",
          "pano_ssc_probe": "ssc", "pano_sobel": "sobel_smooth", "pano_msop_smooth": "sobel_smooth",
          "pano_msop_describe": "describe"}


class StagedLib:
    """The engine's library with every entry point of STAGES waited for and timed: the wall
    seconds from the call to the end of its kernels, added up per stage in ``seconds``."""

    def __init__(self, lib, wait):
        self._lib, self._wait, self.seconds = lib, wait, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        stage = STAGES.get(name)
        if stage is None:
            return fn

        def timed(*args):
            self._wait()
            start = time.perf_counter()
            rc = fn(*args)
            self._wait()
            self.seconds[stage] = self.seconds.get(stage, 0.0) + time.perf_counter() - start
            return rc

        return timed


def time_gpu(frames, repeats):
    sys.path.insert(0, ROOT)
    import torch
    from pano360_amd import engine, features
    eng = engine.engine()
    plain = eng.lib
    out = {}
    for (h, w), img in frames.items():
        frame = eng.upload_frames([img])[0]
        points, _ = features.msop_detect_device(frame, eng=eng)        # warm-up
        whole, stages = [], []
        for _ in range(repeats):
            torch.cuda.synchronize(eng.device)
            start = time.perf_counter()
            features.msop_detect_device(frame, eng=eng)
            torch.cuda.synchronize(eng.device)
            whole.append(time.perf_counter() - start)
        for _ in range(repeats):
            eng.lib = StagedLib(plain, lambda: torch.cuda.synchronize(eng.device))
            try:
                features.msop_detect_device(frame, eng=eng)
                stages.append(eng.lib.seconds)
            finally:
                eng.lib = plain
        out[f"{h}x{w}"] = {
            "points": int(points.shape[0]),
            "whole_ms": round(1e3 * float(np.median(whole)), 3),
            "stage_ms": {k: round(1e3 * float(np.median([s[k] for s in stages])), 3)
                         for k in stages[0]}}
    return out


def time_reference(frames, directory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_msop_golden as gen
    ref = gen.load_reference(directory)
    out = {}
    for (h, w), img in frames.items():
        start = time.perf_counter()
        points, _ = ref.msop_detect(img.copy())
        out[f"{h}x{w}"] = {"points": int(len(points)),
                           "seconds": round(time.perf_counter() - start, 3)}
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reference", help="directory of the reference sources (CPU time)")
    parser.add_argument("--no-gpu", action="store_true", help="skip the GPU timing")
    parser.add_argument("--repeats", type=int, default=5)
    args = parser.parse_args()
    frames = {size: frame_of(*size) for size in SIZES}
    result = {"probe": "msop", "max_feat": [5000, 100, 25, 10]}
    if not args.no_gpu:
        result["gpu"] = time_gpu(frames, args.repeats)
    if args.reference:
        result["reference_cpu"] = time_reference(frames, args.reference)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
