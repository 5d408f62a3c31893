"""Time the bracket deghosting (deghost.deghost_device: one native call for all stacks, 5 launches)
on the frames of the bench: 32 stacks of 3 exposures of 3840 x 2160 and 8 stacks of 3 exposures
of 1920 x 1080, a smooth scene at the gains of a -/0/+ bracket with a mover - a disc - planted in
two of the three exposures, at another place in each - and the fusion of the same stacks beside
it.

Per set, median / min / max over --reps calls after two warm-up calls, in ms, from device events
around the call (the host's share is inside: the records, the output tensors and the workspace
from torch's caching allocator, the launches, and the one wait for the counts; the frames are on
the device before).  ``masks_ms`` is the detection alone (no frame is written), ``deghost_ms`` the
whole stage, ``fuse_ms`` the fusion of the same stacks.  ``kernels_ms`` is each kernel family's
summed device time in one timed call, from the library's own events (the tables go with the raw
masks).  Beside them the bytes the stage must move at the least (``min_bytes``), per pixel of a
frame, and that count over the HBM peak:
  hist      3 read, the grey image (1) written, every frame
  raw       the frame's and the reference's grey (2) read, the raw mask (1/8) written, per frame
            other than the reference; the tables are 2 KB a frame
  clean     the raw mask (1/8) read, the final mask (1/8) written, per frame other than the reference
  apply     3 read, 3 written and the mask (1/8) read per frame whose count is not 0, and 3 of the
            reference for every replaced pixel
Prints one JSON line per set.

    python tools/probe_deghost.py [--reps 10] [--small]"""
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
GAINS = (0.5, 1.0, 2.0)
SPOTS = (0.2, None, 0.7)            # the disc's centre, x over w, per exposure; None: no disc


def min_bytes(h, w, k, counts):
    """The bytes each kernel family moves at the least for one stack: a dict by kernel."""
    n = h * w
    changed = [int(c) for c in counts if c > 0]
    return {"hist": k * 4 * n,
            "raw": (k - 1) * (2 * n + n // 8),
            "clean": (k - 1) * (n // 4),
            "apply": len(changed) * (6 * n + n // 8) + 3 * sum(changed)}


def scene_stacks(n, k, w, h, device):
    """n stacks of k exposures of one smooth scene at the gains of a -/0/+ bracket, unit noise, and
    a bright disc of radius min(h, w) / 8 where SPOTS says."""
    import torch
    gen = torch.Generator(device=device).manual_seed(n)
    coarse = torch.rand((1, 1, h // 16 + 2, w // 16 + 2), device=device, generator=gen)
    scene = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear")[0, 0] * 100.0 + 4.0
    yy = torch.arange(h, device=device)[:, None]
    xx = torch.arange(w, device=device)[None, :]
    stacks = []
    for _ in range(n):
        stack = []
        for e in range(k):
            rad = scene
            spot = SPOTS[e % 3]
            if spot is not None:
                disc = (yy - h // 2) ** 2 + (xx - int(spot * w)) ** 2 <= (min(h, w) // 8) ** 2
                rad = torch.where(disc, torch.full_like(scene, 120.0), scene)
            frame = rad * GAINS[e % 3] + torch.randn((h, w), device=device, generator=gen)
            stack.append(frame.clamp(0, 255).round().to(torch.uint8)[..., None].expand(h, w, 3).contiguous())
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
    from pano360_amd import deghost, engine, fuse
    eng = engine.engine()
    for name, (n, k, w, h) in (SMALL if args.small else SETS).items():
        stacks = scene_stacks(n, k, w, h, eng.device)
        masks_stats, counts = timed(lambda: deghost.masks_device(stacks, None, eng), args.reps)
        deghost_stats, (cleaned, _) = timed(lambda: deghost.deghost_device(stacks, None, eng), args.reps)
        fuse_stats, _ = timed(lambda: fuse.fuse_device(stacks, None, eng), args.reps)
        eng.timing(True)
        deghost.deghost_device(stacks, None, eng)
        kernels = {key: round(ms, 4) for key, (ms, _) in eng.kernel_times().items() if key.startswith("deghost_")}
        eng.timing(False)
        parts = {key: 0 for key in ("hist", "raw", "clean", "apply")}
        for found in counts:
            one = min_bytes(h, w, k, found)
            parts = {key: parts[key] + one[key] for key in parts}
        nbytes = sum(parts.values())
        floor_ms = 1e3 * nbytes / HBM_PEAK
        shares = [float(c) / (h * w) for found in counts for c in found]
        print(json.dumps({"item": name, "stacks": [n, k, w, h], "launches": 5,
                          "changed_frames": sum(int(c > 0) for found in counts for c in found),
                          "max_share_replaced": round(max(shares), 4),
                          "masks_ms": masks_stats, "deghost_ms": deghost_stats, "fuse_ms": fuse_stats,
                          "deghost_over_fuse": round(deghost_stats["median"] / fuse_stats["median"], 4),
                          "kernels_ms": kernels, "bytes": nbytes,
                          "bytes_per_frame_pixel": {key: round(v / (n * k * w * h), 3) for key, v in parts.items()},
                          "hbm_floor_ms": round(floor_ms, 4),
                          "share_of_hbm_peak": round(floor_ms / deghost_stats["median"], 4)}), flush=True)
        del stacks, cleaned
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
