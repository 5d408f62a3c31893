"""Time bundle_adj.traverse on a seeded ring of 32 cameras: 64 pairs (neighbours and second
neighbours) of 2000 matches each, badjust="incr" by default.

Prints one JSON line: the whole traverse (after a warm-up run), the number of LM iterations
and, per iteration, the device time of the normal-equation and residual kernels (HIP events),
the host solve, the time spent waiting for downloads and everything else on the host.

    python tools/probe_bundle.py [--cameras 32] [--matches 2000] [--mode incr] [--model]
--model also times tests/ba_model.py's NumPy traverse on the same input (host only)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--cameras", type=int, default=32)
    parser.add_argument("--matches", type=int, default=2000)
    parser.add_argument("--mode", default="incr", choices=["none", "incr", "last"])
    parser.add_argument("--model", action="store_true")
    args = parser.parse_args()
    import torch
    import ba_model as bm
    from pano360_amd import bundle_adj as ba

    matches, _ = bm.synthetic_matches(2024, args.cameras, args.matches, reach=2)
    n_pairs = sum(len(v) for v in matches.values()) // 2
    imgs = [None] * args.cameras
    ba.traverse(imgs, matches, badjust=args.mode)          # warm-up: library, engine, caches
    torch.cuda.synchronize()

    acc = {"normal_kernels_ms": 0.0, "residual_kernels_ms": 0.0, "solve_ms": 0.0,
           "wait_ms": 0.0}
    events = []
    orig_normal, orig_ssq = ba._Device.normal, ba._Device.pair_ssq
    orig_download, orig_solve = ba._Device.download, np.linalg.solve

    def timed(fn, key):
        def run(self, *a, **kw):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out = fn(self, *a, **kw)
            end.record()
            events.append((key, start, end))
            return out
        return run

    def download(self, *t):
        t0 = time.perf_counter()
        out = orig_download(self, *t)
        acc["wait_ms"] += 1e3 * (time.perf_counter() - t0)
        return out

    def solve(a, b):
        t0 = time.perf_counter()
        out = orig_solve(a, b)
        acc["solve_ms"] += 1e3 * (time.perf_counter() - t0)
        return out

    ba._Device.normal, ba._Device.pair_ssq = timed(orig_normal, "normal"), timed(orig_ssq, "res")
    ba._Device.download, np.linalg.solve = download, solve
    made = []
    orig_cls = ba.IncrementalBundleAdjuster

    class Kept(orig_cls):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    ba.IncrementalBundleAdjuster = Kept
    try:
        t0 = time.perf_counter()
        cams = ba.traverse(imgs, matches, badjust=args.mode)
        total = time.perf_counter() - t0
    finally:
        ba._Device.normal, ba._Device.pair_ssq = orig_normal, orig_ssq
        ba._Device.download, np.linalg.solve = orig_download, orig_solve
        ba.IncrementalBundleAdjuster = orig_cls
    torch.cuda.synchronize()
    for key, start, end in events:
        acc["normal_kernels_ms" if key == "normal" else "residual_kernels_ms"] += \
            start.elapsed_time(end)
    iters = sum(len(h["losses"]) for h in made[0].history)
    per = max(iters, 1)
    out = {"cameras": args.cameras, "pairs": n_pairs, "matches_per_pair": args.matches,
           "mode": args.mode, "cameras_out": len(cams), "traverse_s": round(total, 4),
           "optimize_calls": len(made[0].history), "lm_iterations": iters,
           "per_iteration_ms": {k: round(v / per, 4) for k, v in acc.items()}}
    out["per_iteration_ms"]["total"] = round(1e3 * total / per, 4)
    if args.model:
        t0 = time.perf_counter()
        bm.traverse(args.cameras, matches, args.mode)
        out["model_traverse_s"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
