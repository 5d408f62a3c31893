"""Time the local alignment (csrc/flow.hip, --local-align) beside the stage-level multiband blend
on the same warped patches, in one process, on two rendered rigs of synth.py - 8 frames of
1920 x 1080 over 140 degrees and 32 frames of 3840 x 2160 over 155 degrees, all looking at one
smooth panorama (synth.render_rig) through JITTERED cameras and warped with the unjittered ones, so
that every overlap has something to align - at the resolution cap of the command line
(--max-resolution 1400, the default) or any other (0: native).
Per rig, median / min / max over --reps calls, in ms, from device events around the call (the
host's share of a call is inside: the records and their upload):
  multiband   ownership, blurs, collapse on the unaligned patches
  align       pano_flow_align, the whole stage, into output planes allocated once
  pyramid, search, smooth, apply   the stage's kernel families through their own entry points
and the apply kernel against its byte floor: every pixel of a camera with a partner is read
(16 bytes and a mask byte) and written (16 bytes), a moved pixel reads 16 more, every covering
camera adds an alpha and a mask byte.  Prints one JSON line per rig.

    python tools/probe_flow.py [--reps 10] [--small] [--max-resolution 1400] [--levels 3] [--jitter 0.003]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from probe_view import timed  # noqa: E402


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--small", action="store_true", help="a small scene (a rehearsal)")
    parser.add_argument("--max-resolution", type=int, default=1400, help="0: native")
    parser.add_argument("--levels", type=int, default=3)
    parser.add_argument("--jitter", type=float, default=0.003, help="radians, per axis")
    parser.add_argument("--rigs", default="cfg2,cfg3")
    args = parser.parse_args()
    if args.reps < 1:
        parser.error("--reps is at least 1")

    import torch
    from pano360_amd import engine, flow, synth
    eng = engine.engine()
    cap = args.max_resolution or 10 ** 9
    params = flow.FlowParams(levels=args.levels)
    for name in args.rigs.split(","):
        cfg = dict(synth.CONFIGS[name])
        if args.small:
            cfg.update(width=cfg["width"] // 8, height=cfg["height"] // 8)
        n, w, h = cfg["n"], cfg["width"], cfg["height"]
        rots, intrs = synth.make_cameras(n, w, h, sweep_deg=cfg["sweep_deg"])
        shaken, _ = synth.make_cameras(n, w, h, sweep_deg=cfg["sweep_deg"], jitter=args.jitter, seed=9)
        pano = synth.make_frame(7, 1024 if args.small else 4096, 512 if args.small else 2048, "B")
        frames = synth.render_rig(pano, shaken, intrs, w, h, eng.device)
        plan = eng.upload_plan(engine.Plan([(h, w)] * n, rots, intrs, True, cap))
        levels = cfg["n_levels"]
        patches, _ = eng.warp_all(frames, plan, n_blur=levels - 1)
        del frames
        table = engine.patch_table(patches, eng)
        shape = plan.shape
        H, W = shape
        plain, _ = timed(lambda: eng.multiband(patches, shape, levels, table=table), args.reps)

        lay = flow.Layout(flow.rects_of(patches), params)
        work = torch.empty(lay.total, dtype=torch.uint8, device=eng.device)
        outs = [torch.empty_like(p.planes) if lay.paired[c] else None for c, p in enumerate(patches)]
        ptrs = np.array([0 if t is None else t.data_ptr() for t in outs], np.uint64)
        stats = torch.zeros(4, dtype=torch.int32, device=eng.device)
        native = params.native()
        head = (table.host, table.n, H, W, C.byref(native), work, lay.total)
        ms = {"multiband": plain}
        ms["align"], _ = timed(lambda: eng.call("pano_flow_align", *head, ptrs, None, None, None, stats),
                               args.reps)
        for stage in ("pyramid", "search", "smooth"):
            ms[stage], _ = timed(lambda: eng.call(f"pano_flow_{stage}", *head), args.reps)
        ms["apply"], _ = timed(lambda: eng.call("pano_flow_apply", *head, ptrs, stats), args.reps)
        moved, valid = (int(v) for v in stats[:2].tolist())
        host = np.zeros(lay.total, np.uint8)
        host[lay.vectors_at:lay.stats_at] = work[lay.vectors_at:lay.stats_at].cpu().numpy()
        st = flow.statistics(lay, host, [moved, valid], params)
        pixels = sum(p.h * p.w for c, p in enumerate(patches) if lay.paired[c])
        # covering cameras of a valid pixel: itself and, in an overlap, its partners (counted once
        # per partner rect intersection, an upper estimate of what the mask lets through)
        covering = sum((pr[4] - pr[3]) * (pr[6] - pr[5]) * 2 for pr in lay.pairs)
        floor_bytes = 33 * pixels + 16 * moved + 5 * (valid + covering)
        print(json.dumps({"rig": name, "frames": n, "frame": [w, h], "mosaic": [W, H], "levels": params.levels,
                          "jitter": args.jitter, "ms": ms,
                          "align_to_multiband": round(ms["align"]["median"] / plain["median"], 3),
                          "pairs": st["pairs"], "blocks": st["blocks"], "known": st["known"],
                          "median_px": st["median"], "largest_px": st["largest"], "at_reach": st["at_reach"],
                          "moved": moved, "valid": valid, "patch_pixels": pixels,
                          "workspace_bytes": lay.total, "apply_floor_bytes": floor_bytes,
                          "apply_gb_per_s": round(floor_bytes / ms["apply"]["median"] / 1e6, 1)}), flush=True)
        del patches, table, outs, work


if __name__ == "__main__":
    main()
