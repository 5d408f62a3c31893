"""Time bundle_adj.refine on a seeded ring of 32 cameras: 64 pairs (neighbours and second
neighbours) of 2000 matches each, the matches pushed through the forward radial model
(k1 = -0.08), started from the cameras bundle_adj.traverse makes of them.

Prints one JSON line.  After a warm-up run, refine is run --repeats times: the median, least and
largest whole-call time, the iterations and, per kernel call, the same three figures of the
device time (the upload of the cameras, pano_ba_refine and the copy back, between HIP events),
the host solve, the wait for the download and the total.  Beside it traverse on the same
matches, as tools/probe_bundle.py times it, run --repeats times too: whole and per LM iteration.

    python tools/probe_refine.py [--cameras 32] [--matches 2000] [--lens-terms 1] [--repeats 10]"""
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
    parser.add_argument("--lens-terms", type=int, default=1, choices=[0, 1, 2])
    parser.add_argument("--repeats", type=int, default=10)
    args = parser.parse_args()
    import torch
    import ba_model as bm
    import refine_cases as rc
    from pano360_amd import bundle_adj as ba

    matches, (_, focal) = bm.synthetic_matches(2024, args.cameras, args.matches, reach=2)
    matches = rc.distorted(matches, focal, rc.K_TRUE)
    n_pairs = sum(len(v) for v in matches.values()) // 2
    imgs = [np.full(1, i) for i in range(args.cameras)]

    made = []
    orig_cls = ba.IncrementalBundleAdjuster

    class Kept(orig_cls):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    ba.IncrementalBundleAdjuster = Kept
    try:
        ba.traverse(imgs, matches)                          # warm-up: library, engine, caches
        torch.cuda.synchronize()
        traverse_s = []
        for _ in range(args.repeats):
            del made[:]
            t0 = time.perf_counter()
            cams = ba.traverse(imgs, matches)
            traverse_s.append(time.perf_counter() - t0)
    finally:
        ba.IncrementalBundleAdjuster = orig_cls
    traverse_iters = sum(len(h["losses"]) for h in made[0].history)
    index = [int(c.img[0]) for c in cams]

    ba.refine(cams, matches, index, lens_terms=args.lens_terms)        # warm-up
    torch.cuda.synchronize()
    acc = {"solve_ms": 0.0, "wait_ms": 0.0}
    events = []
    orig_sums, orig_download, orig_solve = ba._Refiner.sums, ba._Device.download, np.linalg.solve

    def sums(self, *a):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = orig_sums(self, *a)
        end.record()
        events.append((start, end))
        return out

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

    def spread(values, digits=4):
        return [round(float(np.median(values)), digits), round(min(values), digits),
                round(max(values), digits)]

    runs = {"refine_s": [], "device_ms": [], "solve_ms": [], "wait_ms": [], "total_ms": []}
    ba._Refiner.sums, ba._Device.download, np.linalg.solve = sums, download, solve
    try:
        for _ in range(args.repeats):
            del events[:]
            acc.update(solve_ms=0.0, wait_ms=0.0)
            t0 = time.perf_counter()
            res = ba.refine(cams, matches, index, lens_terms=args.lens_terms)
            total = time.perf_counter() - t0
            torch.cuda.synchronize()
            calls = max(len(events), 1)
            # (the events bracket the upload of the cameras, the kernel and the download's wait)
            runs["refine_s"].append(total)
            runs["device_ms"].append(sum(a.elapsed_time(b) for a, b in events) / calls)
            runs["solve_ms"].append(acc["solve_ms"] / calls)
            runs["wait_ms"].append(acc["wait_ms"] / calls)
            runs["total_ms"].append(1e3 * total / calls)
    finally:
        ba._Refiner.sums, ba._Device.download, np.linalg.solve = \
            orig_sums, orig_download, orig_solve
    per = max(traverse_iters, 1)
    out = {"cameras": args.cameras, "pairs": n_pairs, "matches_per_pair": args.matches,
           "lens_terms": args.lens_terms, "cameras_in": len(cams), "repeats": args.repeats,
           "figures": "median, min, max", "refine_s": spread(runs["refine_s"]),
           "iterations": len(res.history), "kernel_calls": len(events),
           "accepted": int(sum(h[2] for h in res.history)),
           "rms_before": res.rms_before, "rms_after": res.rms_after,
           "inlier_share": res.inlier_share, "k": res.k,
           "per_call_ms": {k: spread(runs[k]) for k in ("device_ms", "solve_ms", "wait_ms",
                                                         "total_ms")},
           "traverse_s": spread(traverse_s), "traverse_lm_iterations": traverse_iters,
           "traverse_per_iteration_ms": spread([1e3 * t / per for t in traverse_s])}
    print(json.dumps(out))

if __name__ == "__main__":
    main()
