"""Time the device PNG encode (png.encode_device) of a mosaic resident on the device against
what the CLI did before: download the mosaic, reverse the channels and save with Pillow.

Inputs (uint8 BGR on the device): a 1024 x 1024 smooth tile (synth.make_frame, kind B) repeated
to the size, +-3 of noise on every byte, the top and bottom eighth black as a cropped mosaic's
bands are; at 3840x2160, config 3's mosaic size (13760x2474) and config 5's (46079x4948).  Per
input, median and range over --reps runs, in ms:
  device_kernels   the encode's kernels (HIP events around each launch, pano_timing_*)
  device_total     encode_device end to end: the kernels, the waits, the stream's download and
                   the container (the file's bytes in host memory)
  download_pillow  mosaic.cpu(), [..., ::-1], Image.save(BytesIO, "PNG")
and the file size against Pillow's.  Prints one JSON line per input; also checks that the
device's file opens to the mosaic's pixels.

    python tools/probe_png.py [--reps 5] [--pillow-reps 1] [--only NAME]"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INPUTS = {"4k": (3840, 2160), "config3": (13760, 2474), "config5": (46079, 4948)}


def _stats(ms):
    return {"median": round(float(np.median(ms)), 2), "min": round(float(min(ms)), 2),
            "max": round(float(max(ms)), 2)}


def make_mosaic(w, h, device):
    import torch
    from pano360_amd import synth
    tile = torch.from_numpy(synth.make_frame(3, 1024, 1024, "B")).to(device)
    out = tile.repeat(-(-h // 1024), -(-w // 1024), 1)[:h, :w].contiguous()
    gen = torch.Generator(device=device).manual_seed(7)
    noise = torch.randint(-3, 4, out.shape, generator=gen, dtype=torch.int16, device=device)
    out = (out.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)
    out[:h // 8] = 0
    out[h - h // 8:] = 0
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--pillow-reps", type=int, default=1)
    parser.add_argument("--only", default=None)
    args = parser.parse_args()
    if args.reps < 1 or args.pillow_reps < 1:
        parser.error("--reps and --pillow-reps are at least 1")

    import torch
    from PIL import Image
    from pano360_amd import _lib, engine, png
    Image.MAX_IMAGE_PIXELS = None
    eng = engine.engine()
    lib = eng.lib
    names = [lib.pano_kernel_name(k).decode() for k in range(lib.pano_kernel_count())]
    enc_ids = [k for k, n in enumerate(names) if n.startswith(("png_", "deflate_"))]
    for name, (w, h) in INPUTS.items():
        if args.only and name != args.only:
            continue
        mosaic = make_mosaic(w, h, eng.device)
        torch.cuda.synchronize()
        data = png.encode_device(mosaic, eng=eng)                   # warm-up (buffers grow)
        total, kernels, per_kernel = [], [], {}
        for _ in range(args.reps):
            _lib.check(lib.pano_timing_enable(eng.ctx(), 1), "pano_timing_enable")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data = png.encode_device(mosaic, eng=eng)
            total.append(1e3 * (time.perf_counter() - t0))
            ksum = 0.0
            for kid in enc_ids:
                ms, cnt = C.c_double(), C.c_int()
                _lib.check(lib.pano_timing_read(eng.ctx(), kid, C.byref(ms), C.byref(cnt)),
                           "pano_timing_read")
                ksum += ms.value
                per_kernel.setdefault(names[kid], []).append(ms.value)
            kernels.append(ksum)
            _lib.check(lib.pano_timing_enable(eng.ctx(), 0), "pano_timing_enable")
        pil = []
        for _ in range(args.pillow_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = mosaic.cpu().numpy()
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(host[..., ::-1])).save(buf, "PNG")
            pil.append(1e3 * (time.perf_counter() - t0))
        back = np.asarray(Image.open(io.BytesIO(data)))
        rec = {"input": name, "w": w, "h": h, "megapixels": round(w * h / 1e6, 1),
               "bytes": len(data), "pillow_bytes": len(buf.getvalue()),
               "size_ratio": round(len(data) / len(buf.getvalue()), 4),
               "lossless": bool(np.array_equal(back[..., ::-1], host)),
               "device_kernels": _stats(kernels), "device_total": _stats(total),
               "download_pillow": _stats(pil),
               "per_kernel_median": {k: round(float(np.median(v)), 3)
                                     for k, v in per_kernel.items()}}
        rec["speedup_total"] = round(rec["download_pillow"]["median"] /
                                     rec["device_total"]["median"], 1)
        print(json.dumps(rec), flush=True)
        del mosaic, host, back
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
