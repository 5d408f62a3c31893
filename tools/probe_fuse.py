"""Time the exposure fusion (fuse.fuse_device: one native call for all stacks, 3 L + 2 launches per
stack) on the frames of the bench: 32 stacks of 3 exposures of 3840 x 2160 and 8 stacks of 3
exposures of 1920 x 1080.

Per set, median / min / max over --reps calls after two warm-up calls, in ms, from device events
around the call (the host's share is inside: the records, the output tensors and the workspace
from torch's caching allocator, the launches; the frames are on the device before).  Beside the
call's time, the bytes the four kernels must move at the least (``min_bytes``: every level's
pixels read and written once by each kernel that touches them, computed from the shapes) and that
count over the HBM peak:
  pack       3 k bytes read and 16 k written per pixel of the frame
  down       per step 16 k read per pixel of the finer and 16 k written per pixel of the coarser level
  level      16 k read per pixel of the level and of the level below it, 16 written
  collapse   16 read per pixel of the level and of the level below it, 16 written (3 at level 0)
The frames are noise: the values do not change the work.  Prints one JSON line per set.

    python tools/probe_fuse.py [--reps 10] [--small]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from probe_view import HBM_PEAK, timed  # noqa: E402

SETS = {"32x3x4k": (32, 3, 3840, 2160), "8x3x1080p": (8, 3, 1920, 1080)}
SMALL = {"2x3x270p": (2, 3, 480, 270)}


def min_bytes(h, w, k, levels):
    """The bytes each kernel family moves at the least for one stack: a dict by kernel."""
    n = [h * w]
    for _ in range(levels):
        h, w = (h + 1) // 2, (w + 1) // 2
        n.append(h * w)
    out = {"pack": (3 * k + 16 * k) * n[0],
           "down": sum(16 * k * (n[l] + n[l + 1]) for l in range(levels)),
           "level": sum(16 * k * (n[l] + n[l + 1]) + 16 * n[l] for l in range(levels))
           + (16 * k + 16) * n[levels],
           "collapse": sum(16 * (n[l] + n[l + 1]) + 16 * n[l] for l in range(1, levels))}
    out["collapse"] += (16 * (n[0] + n[1]) if levels else 16 * n[0]) + 3 * n[0]
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--small", action="store_true", help="a small set (a rehearsal)")
    args = parser.parse_args()
    if args.reps < 1:
        parser.error("--reps is at least 1")

    import torch
    from pano360_amd import engine, fuse
    eng = engine.engine()
    for name, (n, k, w, h) in (SMALL if args.small else SETS).items():
        gen = torch.Generator(device=eng.device).manual_seed(n)
        stacks = [[torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=eng.device, generator=gen)
                   for _ in range(k)] for _ in range(n)]
        levels = fuse.levels_for(h, w)
        parts = min_bytes(h, w, k, levels)
        nbytes = n * sum(parts.values())
        floor_ms = 1e3 * nbytes / HBM_PEAK
        stats, _ = timed(lambda: fuse.fuse_device(stacks, None, eng), args.reps)
        print(json.dumps({"item": name, "stacks": [n, k, w, h], "levels": levels,
                          "launches": n * (3 * levels + 2 if levels else 3), "ms": stats,
                          "ms_per_stack": round(stats["median"] / n, 4), "bytes": nbytes,
                          "bytes_per_pixel": {key: round(v / (w * h), 2) for key, v in parts.items()},
                          "hbm_floor_ms": round(floor_ms, 4),
                          "share_of_hbm_peak": round(floor_ms / stats["median"], 4)}), flush=True)
        del stacks
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
