"""Time the fused median blend (engine.median_fused) beside the fused linear blend
(engine.blend_fused) in one process, on the bench's config 3 rig (32 frames of 3840 x 2160, a 155
degree sweep at native resolution, unpadded patches) with two sets of frames:
  noise    the bench's frames: unrelated noise, so the samples of a pixel never agree and every
           covered pixel with two or more samples takes the vote - the blender's worst case
  static   the same cameras looking at one smooth panorama (synth.render_rig): a scene in which
           nothing moved, where a pixel's samples agree within the tolerance and the kernel leaves
           after its first walk
Per set and item, median / min / max over --reps runs, in ms, from device events around the call
(the host's share of a call is inside: the two output allocations):
  linear           blend_fused(linear=True)
  none             blend_fused(linear=False)
  median_tol0.1    median_fused at the default tolerance
  median_tol0      median_fused at tol = 0: every pixel whose samples differ at all votes
  median_tol2      median_fused at tol = 2: no pixel votes (the cost of the first walk alone)
each median item with its ratio to `linear`.  Beside them the samples per pixel (mean over the
covered pixels, maximum) and the share of covered pixels with more than PANO_MEDIAN_KEEP samples,
which the kernel consumes in passes; the share of pixels whose median mosaic differs from the
linear one; and the CRC-32 of every mosaic, to compare two builds of the library (PANO_LIB).
Prints one JSON line per item.

    python tools/probe_median.py [--reps 20] [--small] [--sets noise,static]"""
import argparse
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from probe_view import timed  # noqa: E402


def rig(small):
    from pano360_amd import synth
    cfg = dict(n=8, width=480, height=270, sweep_deg=140.0) if small else synth.CONFIGS["cfg3"]
    rots, intrs = synth.make_cameras(cfg["n"], cfg["width"], cfg["height"],
                                     sweep_deg=cfg.get("sweep_deg"))
    return cfg, rots, intrs


def frames_of(kind, cfg, rots, intrs, eng, small):
    from pano360_amd import synth
    if kind == "noise":
        return [eng.upload_frames([synth.make_frame(i, cfg["width"], cfg["height"], "A")])[0]
                for i in range(cfg["n"])]
    pano = synth.make_frame(7, 1024 if small else 4096, 512 if small else 2048, "B")
    return synth.render_rig(pano, rots, intrs, cfg["width"], cfg["height"], eng.device)


def sample_counts(eng, frames, plan):
    """Samples per mosaic pixel (int32 [H][W] on the device) from the masks of the warped patches."""
    import torch
    counts = torch.zeros(plan.shape, dtype=torch.int32, device=eng.device)
    patches, _ = eng.warp_all(frames, plan)
    for dp in patches:
        y0, y1, x0, x1 = dp.rect
        counts[y0:y1, x0:x1] += (dp.mask == 0).to(torch.int32)
    return counts


def crc(mosaic):
    return zlib.crc32(mosaic.cpu().numpy().tobytes())


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--small", action="store_true", help="a small scene (a rehearsal)")
    parser.add_argument("--sets", default="noise,static")
    args = parser.parse_args()
    sets = args.sets.split(",")
    if args.reps < 1 or not set(sets) <= {"noise", "static"}:
        parser.error("--reps is at least 1, --sets of noise and static")

    import torch
    from pano360_amd import _lib, engine
    eng = engine.engine()
    cfg, rots, intrs = rig(args.small)
    plan = engine.Plan([(cfg["height"], cfg["width"])] * cfg["n"], rots, intrs, False, 10 ** 9)
    eng.upload_plan(plan)
    H, W = plan.shape
    for kind in sets:
        frames = frames_of(kind, cfg, rots, intrs, eng, args.small)
        counts = sample_counts(eng, frames, plan)
        covered = int((counts > 0).sum())
        scene = {"set": kind, "mosaic": [W, H], "frames": cfg["n"],
                 "samples_mean": round(float(counts.sum(dtype=torch.int64)) / max(covered, 1), 2),
                 "samples_max": int(counts.max()),
                 "share_above_keep": round(int((counts > _lib.MEDIAN_KEEP).sum()) / max(covered, 1), 6)}
        del counts
        torch.cuda.synchronize()
        base, (linear, _) = timed(lambda: eng.blend_fused(frames, plan, True), args.reps)
        print(json.dumps({"item": "linear", **scene, "ms": base, "crc32": crc(linear)}), flush=True)
        stats, (mosaic, _) = timed(lambda: eng.blend_fused(frames, plan, False), args.reps)
        print(json.dumps({"item": "none", **scene, "ms": stats, "crc32": crc(mosaic)}), flush=True)
        for tol in (0.1, 0.0, 2.0):
            stats, (mosaic, _) = timed(lambda t=tol: eng.median_fused(frames, plan, t), args.reps)
            differs = int((mosaic != linear).any(dim=-1).sum())
            print(json.dumps({"item": f"median_tol{tol:g}", **scene, "ms": stats,
                              "ratio_to_linear": round(stats["median"] / base["median"], 3),
                              "share_differs_from_linear": round(differs / (H * W), 6),
                              "crc32": crc(mosaic)}),
                  flush=True)
        del frames, linear, mosaic


if __name__ == "__main__":
    main()
