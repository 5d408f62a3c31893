"""Time the view stage (view.mip_device, view.render_device) on the mosaic of the bench's
config 3 scene (32 frames of 3840 x 2160, a 155 degree sweep at native resolution).

Per item, median / min / max over --reps runs, in ms, from device events around the call (the
host's share of a call is inside: allocation of the outputs, the argument records):
  mip_chain      the chain of the mosaic (one copy, one launch per level)
  view_1080p     one 1920 x 1080 look, fov 90 degrees, at the mosaic's centre
  cube_2048      six 2048 x 2048 faces, one launch
  equirect_8192  one 8192 x 4096 full-sphere image
Beside each time: the bytes the item must move at the least and that count over the HBM peak.
  mip_chain   reads the mosaic and every level but the last once, writes every level once
  a view      writes 4 bytes per output pixel (image and mask) and reads, per COVERED pixel, 3
              bytes of its lower level and a quarter of that of the upper one (a texel per pixel
              at the pixel's own scale; neighbours share the other taps)
--model also times the NumPy model (tests/view_model.py) on a reduced size: the level-3 image of
the mosaic with its geometry and a 240 x 135 look.  Prints one JSON line per item.

    python tools/probe_view.py [--reps 20] [--model] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12                   # bytes / s (MI355X, specification)


def _stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4),
            "max": round(float(max(ms)), 4)}


def bench_mosaic(eng, small):
    """(device mosaic, MosaicGeometry) of config 3 (--small: 8 frames of 480 x 270)."""
    from pano360_amd import engine, synth, view
    cfg = dict(n=8, width=480, height=270, sweep_deg=140.0, n_levels=5) if small \
        else synth.CONFIGS["cfg3"]
    rots, intrs = synth.make_cameras(cfg["n"], cfg["width"], cfg["height"],
                                     sweep_deg=cfg.get("sweep_deg"))
    plan = engine.Plan([(cfg["height"], cfg["width"])] * cfg["n"], rots, intrs, True, 10 ** 9)
    frames = [eng.upload_frames([synth.make_frame(i, cfg["width"], cfg["height"], "A")])[0]
              for i in range(cfg["n"])]
    eng.upload_plan(plan)
    mosaic = eng.stitch(frames, plan, "multiband", cfg["n_levels"])[0].clone()
    return mosaic, view.MosaicGeometry.of_plan(plan)


def timed(call, reps):
    import torch
    call()                                          # warm-up: code objects, the allocator's blocks
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return _stats(ms), out


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reps", type=int, default=20)
    parser.add_argument("--model", action="store_true")
    parser.add_argument("--small", action="store_true", help="a small scene (a rehearsal)")
    args = parser.parse_args()
    if args.reps < 1:
        parser.error("--reps is at least 1")

    import torch
    from pano360_amd import engine, view
    eng = engine.engine()
    mosaic, geom = bench_mosaic(eng, args.small)
    H, W = geom.shape
    torch.cuda.synchronize()
    centre = (geom.low[0] + geom.resolution[0] * W / 2, -(geom.low[1] + geom.resolution[1] * H / 2))
    shapes = view.mip_shapes(H, W)
    level_bytes = [3 * a * b for a, b in shapes]
    stats, mips = timed(lambda: view.mip_device(mosaic, eng), args.reps)
    items = [("mip_chain", stats, 2 * level_bytes[0] + sum(level_bytes[:-1]) + sum(level_bytes[1:]),
              {"levels": len(shapes)})]
    scale = 8 if args.small else 1
    batches = {"view_1080p": [view.perspective(centre[0], centre[1], 0.0, np.pi / 2,
                                               (1920 // scale, 1080 // scale))],
               "cube_2048": view.cube_faces(2048 // scale),
               "equirect_8192": [view.equirect(8192 // scale)]}
    for name, views in batches.items():
        stats, (_, masks) = timed(lambda v=views: view.render_device(mips, geom, v, eng), args.reps)
        pixels = sum(v.w * v.h for v in views)
        covered = int(sum(int(m.sum(dtype=torch.int64)) for m in masks))
        items.append((name, stats, 4 * pixels + covered * 3 * 5 // 4,
                      {"pixels": pixels, "covered": covered}))
    for name, stats, nbytes, extra in items:
        floor_ms = 1e3 * nbytes / HBM_PEAK
        print(json.dumps({"item": name, "mosaic": [W, H], "ms": stats, "bytes": nbytes,
                          "hbm_floor_ms": round(floor_ms, 4),
                          "share_of_hbm_peak": round(floor_ms / stats["median"], 4), **extra}),
              flush=True)
    if args.model:
        import view_model as vm
        level = min(3, len(shapes) - 1)
        small = mips.level(level).cpu().numpy()
        res = tuple(r * (1 << level) for r in geom.resolution)
        low = tuple(lo + r * ((1 << level) - 1) / 2 for lo, r in zip(geom.low, geom.resolution))
        small_geom = view.MosaicGeometry(low, res, small.shape[:2])
        look = view.perspective(centre[0], centre[1], 0.0, np.pi / 2, (240, 135))
        t0 = time.perf_counter()
        levels = vm.mip_levels(small)
        t1 = time.perf_counter()
        vm.render(levels, small_geom, look)
        t2 = time.perf_counter()
        print(json.dumps({"item": "numpy_model", "mosaic": list(small.shape[1::-1]),
                          "view": [240, 135], "mip_ms": round(1e3 * (t1 - t0), 1),
                          "render_ms": round(1e3 * (t2 - t1), 1),
                          "render_ns_per_pixel": round(1e9 * (t2 - t1) / (240 * 135), 1)}), flush=True)


if __name__ == "__main__":
    main()
