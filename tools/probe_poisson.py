"""Time blend.poisson_blend_device on an overlap-sized blend: 1080 x 976 x 3 seeded textured
images, a half-plane-with-wiggle mask (tests/poisson_model.seam_mask) that covers about half the
pixels and touches the top, the bottom and the right edge.

Prints one JSON line: iterations per channel, ms per blend (device events around the call, after
a warm-up blend), ms per iteration, the bytes an iteration has to move (from the shapes: per
element of a wave that holds a mask pixel the three vector kernels read 10 and write 5 float64
values and read the mask byte three times; elsewhere only the mask byte is read) and the rate
that makes against the HBM peak the bench uses - a yardstick only: the working set of six
vectors stays in the last-level cache - and the time of SciPy's direct solve of the same
systems on this machine's CPU, which is the reference's path (--no-cpu skips it).

    python tools/probe_poisson.py [--height 1080] [--width 976] [--channels 3] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBPS = 8000.0          # bench.py's figure: HBM3E 8 TB/s spec
WAVE_ELEMS = 128                # elements a wave takes per pass (csrc/poisson.hip)
TILE = 2048                     # elements per block


def bytes_per_iteration(mask, channels):
    n = mask.size
    padded = -(-n // TILE) * TILE
    flat = np.zeros(padded, bool)
    flat[:n] = mask.reshape(-1)
    active = int(flat.reshape(-1, WAVE_ELEMS).any(axis=1).sum()) * WAVE_ELEMS
    return channels * (active * (15 * 8 + 3) + (n - min(active, n)) * 3)


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--height", type=int, default=1080)
    parser.add_argument("--width", type=int, default=976)
    parser.add_argument("--channels", type=int, default=3)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--no-cpu", action="store_true")
    args = parser.parse_args()
    import torch
    import poisson_model as pm
    from pano360_amd import blend, engine

    H, W, C = args.height, args.width, args.channels
    src, tgt = pm.textured(H, W, C, 61), pm.textured(H, W, C, 62)
    mask = pm.seam_mask(H, W, 13)
    eng = engine.engine()
    dev_src = torch.from_numpy(src).to(eng.device)
    dev_mask = torch.from_numpy(mask).to(eng.device)

    def run():
        dev_tgt = torch.from_numpy(tgt).to(eng.device)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = blend.poisson_blend_device(dev_src, dev_tgt, dev_mask, eng, want_solution=True)
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end), out

    run()                                                   # warm-up: library, scratch
    times, out = [], None
    for _ in range(args.repeats):
        ms, out = run()
        times.append(ms)
    _, solution, iters, resid = out
    ms = float(np.median(times))
    per_iter = ms / int(iters.max())
    moved = bytes_per_iteration(mask, C)
    # the channels run in the same launches: an iteration lasts as long as there is a channel left
    line = {"probe": "poisson", "shape": [H, W, C], "mask_share": round(float(mask.mean()), 4),
            "iterations": iters.tolist(), "residuals": [float(f"{v:.3e}") for v in resid],
            "ms_per_blend": round(ms, 3), "ms_all": [round(v, 3) for v in times],
            "ms_per_iteration": round(per_iter, 5),
            "mbytes_per_iteration": round(moved / 1e6, 2),
            "gbytes_per_s": round(moved / (per_iter * 1e-3) / 1e9, 1),
            "share_of_hbm_peak": round(moved / (per_iter * 1e-3) / 1e9 / HBM_PEAK_GBPS, 3)}
    if not args.no_cpu:
        t0 = time.perf_counter()
        ref_sol, _ = pm.solve(src, tgt, mask)
        line["cpu_direct_solve_s"] = round(time.perf_counter() - t0, 2)
        line["max_abs_deviation"] = float(f"{np.abs(solution.cpu().numpy() - ref_sol).max():.3e}")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
