"""Time the bracket alignment (align.align_device: one native call for all stacks, 6 + L launches)
on the frames of the bench: 32 stacks of 3 exposures of 3840 x 2160 and 8 stacks of 3 exposures
of 1920 x 1080, a smooth scene cropped at planted shifts - and the fusion of the same stacks
beside it.

Per set, median / min / max over --reps calls after two warm-up calls, in ms, from device events
around the call (the host's share is inside: the records, the output tensors and the workspace
from torch's caching allocator, the launches, and the one wait for the shifts; the frames are on
the device before).  ``shifts_ms`` is the search alone (no frame is copied), ``align_ms`` the whole
stage, ``fuse_ms`` the fusion of the same stacks.  ``kernels_ms`` is each kernel family's summed
device time in one timed call, from the library's own events (the medians go with the bitmaps, the
final shifts with the search).  Beside them the bytes the stage must move at the least
(``min_bytes``), per pixel of a frame, and that count over the HBM peak:
  grey      3 read, the grey pyramid (4/3) written
  bitmap    the pyramid (4/3) read, two bitmaps of every level (1/3) written
  search    the reference's and the frame's two bitmaps of every level (2/3) read, per moved frame
  apply     3 read and 3 written per frame whose shift is not zero
Prints one JSON line per set.

    python tools/probe_align.py [--reps 10] [--small]"""
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
PLANTS = ((13, -7), (-22, 9), (5, 31), (-3, -2), (40, 17), (0, 1))
GAINS = (0.5, 1.0, 2.0)


def min_bytes(h, w, k, levels, moved):
    """The bytes each kernel family moves at the least for one stack: a dict by kernel."""
    n = [(h >> l) * (w >> l) for l in range(levels + 1)]
    return {"grey": k * (3 * n[0] + sum(n)),
            "bitmap": k * (sum(n) + sum(n) // 4),
            "search": (k - 1) * 2 * (sum(n) // 4),
            "apply": moved * 6 * n[0]}


def scene_stacks(n, k, w, h, device):
    """n stacks of k crops of one smooth scene at planted shifts and the gains of a -/0/+ bracket."""
    import torch
    margin = 48
    gen = torch.Generator(device=device).manual_seed(n)
    coarse = torch.rand((1, 1, (h + 2 * margin) // 16 + 2, (w + 2 * margin) // 16 + 2), device=device, generator=gen)
    scene = torch.nn.functional.interpolate(coarse, size=(h + 2 * margin, w + 2 * margin), mode="bilinear")[0, 0]
    scene = scene * 120.0 + 4.0
    stacks, at = [], 0
    for _ in range(n):
        stack = []
        for e in range(k):
            dx, dy = (0, 0) if e == k // 2 else PLANTS[at % len(PLANTS)]
            at += e != k // 2
            crop = scene[margin + dy:margin + dy + h, margin + dx:margin + dx + w] * GAINS[e % 3]
            crop = crop + torch.randn((h, w), device=device, generator=gen)
            stack.append(crop.clamp(0, 255).round().to(torch.uint8)[..., None].expand(h, w, 3).contiguous())
        stacks.append(stack)
    return stacks


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--small", action="store_true", help="a small set (a rehearsal)")
    args = parser.parse_args()
    if args.reps < 1:
        parser.error("--reps is at least 1")

    import torch
    from pano360_amd import align, engine, fuse
    eng = engine.engine()
    for name, (n, k, w, h) in (SMALL if args.small else SETS).items():
        stacks = scene_stacks(n, k, w, h, eng.device)
        levels = align.levels_for(h, w)
        shifts_stats, shifts = timed(lambda: align.shifts_device(stacks, None, eng), args.reps)
        align_stats, (aligned, _) = timed(lambda: align.align_device(stacks, None, eng), args.reps)
        fuse_stats, _ = timed(lambda: fuse.fuse_device(stacks, None, eng), args.reps)
        moved = sum(int(s.any()) for found in shifts for s in found)
        eng.timing(True)
        align.align_device(stacks, None, eng)
        kernels = {key: round(ms, 4) for key, (ms, _) in eng.kernel_times().items() if key.startswith("align_")}
        eng.timing(False)
        parts = {key: 0 for key in ("grey", "bitmap", "search", "apply")}
        for found in shifts:
            one = min_bytes(h, w, k, levels, sum(int(s.any()) for s in found))
            parts = {key: parts[key] + one[key] for key in parts}
        nbytes = sum(parts.values())
        floor_ms = 1e3 * nbytes / HBM_PEAK
        print(json.dumps({"item": name, "stacks": [n, k, w, h], "levels": levels, "launches": 6 + levels,
                          "moved_frames": moved, "max_shift": int(max(abs(found).max() for found in shifts)),
                          "shifts_ms": shifts_stats, "align_ms": align_stats, "fuse_ms": fuse_stats,
                          "align_over_fuse": round(align_stats["median"] / fuse_stats["median"], 4),
                          "kernels_ms": kernels, "bytes": nbytes,
                          "bytes_per_frame_pixel": {key: round(v / (n * k * w * h), 3) for key, v in parts.items()},
                          "hbm_floor_ms": round(floor_ms, 4),
                          "share_of_hbm_peak": round(floor_ms / align_stats["median"], 4)}), flush=True)
        del stacks, aligned
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
