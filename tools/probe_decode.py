"""Time the device JPEG decode of 32 x 3840x2160 frames (synth.make_frame, kind A, one seed per
frame) against Pillow, in three encodings: quality 90 4:2:0, quality 95 4:4:4, and quality 95
4:4:4 with a restart marker every MCU row.

Per encoding, median and range over --reps runs, in ms for the whole batch:
  device_with_upload  jpeg.decode_device from the bytes in memory: parse, pack, one upload of the
                      compressed batch, the native call (waited for)
  device_resident     the native call alone, the packed batch already on the device
  pillow_upload       Image.open + convert("RGB") per file, then the raw BGR upload
and the number of Huffman synchronisation rounds.  Prints one JSON line per encoding.

    python tools/probe_decode.py [--frames 32] [--reps 5] [--pillow-reps 2] [--only NAME]
The per-kernel split comes from a separate run under
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/probe_decode.py --reps 2"""
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

CONFIGS = {"q90_420": dict(quality=90, subsampling=2),
           "q95_444": dict(quality=95, subsampling=0),
           "q95_444_rst": dict(quality=95, subsampling=0, restart_marker_rows=1)}


def _stats(ms):
    return {"median": round(float(np.median(ms)), 2), "min": round(float(min(ms)), 2),
            "max": round(float(max(ms)), 2)}


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--frames", type=int, default=32)
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--pillow-reps", type=int, default=2)
    parser.add_argument("--only", choices=sorted(CONFIGS))
    args = parser.parse_args()
    import torch
    from PIL import Image
    from pano360_amd import _lib, engine, synth
    from pano360_amd import jpeg as J

    eng = engine.engine()
    dev = torch.device(eng.device)
    frames = [synth.make_frame(s, 3840, 2160, "A") for s in range(args.frames)]
    for name, kw in CONFIGS.items():
        if args.only and name != args.only:
            continue
        blobs = []
        for f in frames:
            buf = io.BytesIO()
            Image.fromarray(f).save(buf, "JPEG", **kw)
            blobs.append(buf.getvalue())
        J.decode_device(blobs[:2], eng)                    # warm-up
        torch.cuda.synchronize()
        with_upload = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            J.decode_device(blobs, eng)
            torch.cuda.synchronize()
            with_upload.append(1e3 * (time.perf_counter() - t0))

        headers = [J.parse(b) for b in blobs]
        desc, layout, packed_bytes = J.pack(headers, blobs)
        host = torch.empty(packed_bytes, dtype=torch.uint8, pin_memory=True)
        J.fill_packed(host.numpy(), desc, layout, headers, blobs)
        packed = host.to(dev)
        bt = desc[len(blobs)]
        work = torch.empty(int(bt[J.JB_WORK_BYTES]), dtype=torch.uint8, device=dev)
        out = torch.empty(int(bt[J.JB_OUT_BYTES]), dtype=torch.uint8, device=dev)
        desc_c = np.ascontiguousarray(desc)

        def run():
            _lib.check(eng.lib.pano_jpeg_decode(
                eng.ctx(), desc_c.ctypes.data_as(C.c_void_p), len(blobs), engine._ptr(packed),
                C.c_int64(packed_bytes), engine._ptr(work), C.c_int64(work.numel()),
                engine._ptr(out), C.c_int64(out.numel())), "pano_jpeg_decode")
        resident = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            resident.append(1e3 * (time.perf_counter() - t0))
        _lib.check(eng.lib.pano_timing_enable(eng.ctx(), 1), "pano_timing_enable")
        run()
        torch.cuda.synchronize()
        ms, cnt = C.c_double(0), C.c_int(0)
        names = [eng.lib.pano_kernel_name(k).decode() for k in range(eng.lib.pano_kernel_count())]
        kid = names.index("jpeg_huff_sync_kernel")
        _lib.check(eng.lib.pano_timing_read(eng.ctx(), kid, C.byref(ms), C.byref(cnt)),
                   "pano_timing_read")
        rounds = cnt.value - 1
        _lib.check(eng.lib.pano_timing_enable(eng.ctx(), 0), "pano_timing_enable")

        pil = []
        for _ in range(args.pillow_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in blobs:
                a = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))[..., ::-1])
                torch.from_numpy(a).to(dev)
            torch.cuda.synchronize()
            pil.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps({"config": name, "frames": len(blobs),
                          "jpeg_mb": round(sum(map(len, blobs)) / 1e6, 1),
                          "sync_rounds": rounds,
                          "device_with_upload_ms": _stats(with_upload),
                          "device_resident_ms": _stats(resident),
                          "pillow_upload_ms": _stats(pil) if pil else None}), flush=True)


if __name__ == "__main__":
    main()
