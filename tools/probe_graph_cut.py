"""Time blend.graph_cut_device at the size of the reference main()'s overlap: 1080 x 976 x 3
seeded smooth int16 images (tests/graph_cut_model.smooth_pair), shrink=5 (a 216 x 195 grid, the
resident flood) and shrink=1 (1.05 M cells, the tiled flood).

Prints one JSON line per shrink: the median over --repeats runs, after a warm-up run, of the
whole call and of its three stages timed on their own (device events around each; the whole call
includes its one-word readback; ``flood_tiled`` is the flood forced onto the tiled path), the
flood's own counters - classes (level, colour) that labelled a cell, the passes (resident: a pass is one sweep of the rows or of the columns) or rounds (tiled:
one launch over all tiles) that labelled one, the most of them in a single class - and the time
of the reference's algorithm, the heap loop of tests/graph_cut_model.py, on this machine's CPU
(--no-cpu skips it; there is no other baseline).  ``structure_ok`` is the one condition on the
flood: the passes (rounds) of the worst class stay under 100 - a flood that moved one cell per
sweep would need hundreds.

    python tools/probe_graph_cut.py [--height 1080] [--width 976] [--repeats 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, repeats, fn):
    """Median milliseconds of fn() over `repeats` runs (device events), after one warm-up."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        out.append(start.elapsed_time(stop))
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--height", type=int, default=1080)
    parser.add_argument("--width", type=int, default=976)
    parser.add_argument("--repeats", type=int, default=7)
    parser.add_argument("--no-cpu", action="store_true")
    args = parser.parse_args()
    import torch
    import graph_cut_model as gm
    from pano360_amd import blend, engine

    H, W = args.height, args.width
    img1, img2 = gm.smooth_pair(H, W, 3, 2024, np.int16, noise=2.0)
    eng = engine.engine()
    dev1, dev2 = torch.from_numpy(img1).to(eng.device), torch.from_numpy(img2).to(eng.device)
    for shrink in (5, 1):
        border = blend.seam_border(shrink)
        level, _ = blend.seam_levels_device(dev1, dev2, shrink, eng)
        labels, stats = blend.seam_flood_device(level, border, eng, want_stats=True)
        stats = stats.cpu().numpy().tolist()
        want = gm.flood_sweep(gm.levels(img1, img2, shrink), border)
        record = {
            "shrink": shrink, "grid": list(level.shape),
            "path": {1: "resident", 2: "tiled"}[stats[3]],
            "labels_equal_model": bool(np.array_equal(labels.cpu().numpy(), want)),
            "classes_with_frontier": stats[0],
            "passes_or_rounds": stats[1], "most_in_one_class": stats[2],
            "mean_per_class": round(stats[1] / max(stats[0], 1), 2),
            "structure_ok": stats[2] < 100,
        }
        for name, fn in (
                ("call", lambda: blend.graph_cut_device(dev1, dev2, shrink, eng)),
                ("levels", lambda: blend.seam_levels_device(dev1, dev2, shrink, eng)),
                ("flood", lambda: blend.seam_flood_device(level, border, eng)),
                ("flood_tiled", lambda: blend.seam_flood_device(level, border, eng, path=2)),
                ("mask", lambda: blend.seam_mask_device(labels, H, W, eng))):
            med, lo, hi = timed(torch, args.repeats, fn)
            record[f"{name}_ms"] = round(med, 4)
            record[f"{name}_ms_range"] = [round(lo, 4), round(hi, 4)]
        if not args.no_cpu:
            lev = gm.levels(img1, img2, shrink)
            start = time.perf_counter()
            heap = gm.flood_heap(lev, border)
            record["cpu_heap_loop_ms"] = round(1e3 * (time.perf_counter() - start), 1)
            record["heap_equals_sweep"] = bool(np.array_equal(heap, want))
        print(json.dumps(record), flush=True)


if __name__ == "__main__":
    main()
