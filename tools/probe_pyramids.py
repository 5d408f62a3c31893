"""Time the two tile pyramids (pano360_amd/tiles.py) of a mosaic resident on the device: the one
batched encode (jpeg.encode_batch_device) against the same tiles through a loop of
jpeg.encode_device, which was the only way to code them before the batch existed.

Input (synth.make_frame, kind B, uint8 BGR on the device): a mosaic of config 3's size
(13760x2474), taken as a closed ring for the cube.  Sets: the full Deep Zoom pyramid and a
``--multires 4096`` cube, both at tile 512, Pillow's defaults (quality 75, 4:2:0).  Per set, median
and range over --reps runs after a warm-up, in ms:
  render         the pixels: the mip chain (Deep Zoom) or the chain and the cube levels' faces
  batch_kernels  the batched encode's kernels (HIP events around each launch, pano_timing_*),
                 in runs of their own
  batch_total    encode_batch_device end to end: kernels, two waits, one download, the headers
  loop_total     [encode_device(tile) for tile in tiles]
  write_files    the files written to a temporary directory
and the tile count, the megapixels and the bytes.  Prints one JSON line per set; also checks that
the two ways give the same files.

    python tools/probe_pyramids.py [--reps 5] [--tile 512] [--side 4096] [--only deepzoom|multires]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MOSAIC = (13760, 2474)


def _stats(ms):
    return {"median": round(float(np.median(ms)), 2), "min": round(float(min(ms)), 2),
            "max": round(float(max(ms)), 2)}


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--tile", type=int, default=512)
    parser.add_argument("--side", type=int, default=4096)
    parser.add_argument("--only", default=None, choices=["deepzoom", "multires"])
    args = parser.parse_args()

    import torch
    from pano360_amd import _lib, engine, jpeg, synth, tiles, view
    eng = engine.engine()
    lib = eng.lib
    names = [lib.pano_kernel_name(k).decode() for k in range(lib.pano_kernel_count())]
    enc_ids = [k for k, n in enumerate(names) if n.startswith("jpeg_enc_")]
    w, h = MOSAIC
    mosaic = torch.from_numpy(synth.make_frame(3, w, h, "B")).to(eng.device)
    res = 2 * math.pi / w
    geom = view.MosaicGeometry((-math.pi, -(h - 1) / 2 * res), (res, res), (h, w))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    def make(which):
        mips = view.mip_device(mosaic, eng)
        if which == "deepzoom":
            return tiles.deepzoom_tiles(mips, args.tile)
        return tiles.multires_tiles(mips, geom, args.side, args.tile, eng)

    for which in ("deepzoom", "multires"):
        if args.only and which != args.only:
            continue
        (tile_names, views), _ = timed(lambda: make(which))          # warm-up
        batch = jpeg.encode_batch_device(views, eng=eng)             # warm-up (buffers grow)
        loop = [jpeg.encode_device(v, eng=eng) for v in views]
        render, total, kernels, looped, written, per_kernel = [], [], [], [], [], {}
        for _ in range(args.reps):
            (tile_names, views), ms = timed(lambda: make(which))
            render.append(ms)
            batch, ms = timed(lambda: jpeg.encode_batch_device(views, eng=eng))
            total.append(ms)
            loop, ms = timed(lambda: [jpeg.encode_device(v, eng=eng) for v in views])
            looped.append(ms)
            _lib.check(lib.pano_timing_enable(eng.ctx(), 1), "pano_timing_enable")
            jpeg.encode_batch_device(views, eng=eng)
            ksum = 0.0
            for kid in enc_ids:
                ms, cnt = C.c_double(), C.c_int()
                _lib.check(lib.pano_timing_read(eng.ctx(), kid, C.byref(ms), C.byref(cnt)),
                           "pano_timing_read")
                ksum += ms.value
                per_kernel.setdefault(names[kid], []).append(ms.value)
            kernels.append(ksum)
            _lib.check(lib.pano_timing_enable(eng.ctx(), 0), "pano_timing_enable")
            with tempfile.TemporaryDirectory() as tmp:
                paths = [os.path.join(tmp, *n.split("/")) for n in tile_names]
                _, ms = timed(lambda: tiles._write_files(paths, batch))
                written.append(ms)
        pixels = sum(int(v.shape[0]) * int(v.shape[1]) for v in views)
        rec = {"set": which, "mosaic": [w, h], "tile": args.tile, "tiles": len(views),
               "megapixels": round(pixels / 1e6, 1), "bytes": sum(len(b) for b in batch),
               "identical": batch == loop, "render": _stats(render),
               "batch_kernels": _stats(kernels), "batch_total": _stats(total),
               "loop_total": _stats(looped), "write_files": _stats(written),
               "per_kernel_median": {k: round(float(np.median(v)), 3)
                                     for k, v in per_kernel.items()}}
        if which == "multires":
            rec["side"] = tiles.multires_levels(args.side, args.tile)[0]
        rec["speedup_total"] = round(rec["loop_total"]["median"] / rec["batch_total"]["median"], 1)
        rec["faster_beyond_spread"] = rec["batch_total"]["max"] < rec["loop_total"]["min"]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
