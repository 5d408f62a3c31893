"""Time the stage-level multiband blend (engine.multiband) beside the seam-routed one
(engine.seam_multiband, -b seam) on the same warped patches, in one process, on two rendered rigs
of synth.py - 8 frames of 1920 x 1080 over 140 degrees and 32 frames of 3840 x 2160 over 155
degrees, all looking at one smooth panorama (synth.render_rig), with a rectangle painted into
every second frame so that the frames disagree somewhere - at the resolution cap of the command
line (--max-resolution 1400, the default) or any other (0: native).
Per rig, median / min / max over --reps runs, in ms, from device events around the call (the
host's share of a call is inside: the output allocations, and for the route its reads of "done"
and its download of the pair matrix):
  multiband        ownership, blurs, collapse
  seam_multiband   seam_route, blurs, collapse
  seam_route       ownership, prepare, colouring, flood, finish alone
and the route's counters: classes and rounds that labelled a pixel, the most rounds in one class,
pixels whose owner changed, open pixels, groups.  Prints one JSON line per rig.

    python tools/probe_seam_route.py [--reps 10] [--small] [--max-resolution 1400] [--ratio 0.5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from probe_view import timed  # noqa: E402


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reps", type=int, default=10)
    parser.add_argument("--small", action="store_true", help="a small scene (a rehearsal)")
    parser.add_argument("--max-resolution", type=int, default=1400, help="0: native")
    parser.add_argument("--ratio", type=float, default=0.5)
    parser.add_argument("--rigs", default="cfg2,cfg3")
    args = parser.parse_args()
    if args.reps < 1:
        parser.error("--reps is at least 1")

    import torch
    from pano360_amd import engine, synth
    eng = engine.engine()
    cap = args.max_resolution or 10 ** 9
    for name in args.rigs.split(","):
        cfg = dict(synth.CONFIGS[name])
        if args.small:
            cfg.update(width=cfg["width"] // 8, height=cfg["height"] // 8)
        n, w, h = cfg["n"], cfg["width"], cfg["height"]
        rots, intrs = synth.make_cameras(n, w, h, sweep_deg=cfg["sweep_deg"])
        pano = synth.make_frame(7, 1024 if args.small else 4096, 512 if args.small else 2048, "B")
        frames = synth.render_rig(pano, rots, intrs, w, h, eng.device)
        for k in range(1, n, 2):                    # what only this frame shows
            frames[k][h // 3:h // 2, 5 * w // 8:3 * w // 4] = torch.tensor(
                [250, 20, 230], dtype=torch.uint8, device=eng.device)
        plan = eng.upload_plan(engine.Plan([(h, w)] * n, rots, intrs, True, cap))
        levels = cfg["n_levels"]
        patches, _ = eng.warp_all(frames, plan, n_blur=levels - 1)
        table = engine.patch_table(patches, eng)
        shape = plan.shape
        plain, out = timed(lambda: eng.multiband(patches, shape, levels, table=table), args.reps)
        argmax = out[2]
        routed, out = timed(lambda: eng.seam_multiband(patches, shape, levels, args.ratio,
                                                       table=table), args.reps)
        valid = int(out[3].sum())
        differs = int((out[2] != argmax).sum())
        alone, out = timed(lambda: eng.seam_route(table, shape, args.ratio), args.reps)
        stats = out[2].tolist()
        assert differs == stats[3]
        print(json.dumps({"rig": name, "frames": n, "frame": [w, h], "mosaic": [shape[1], shape[0]],
                          "levels": levels, "ratio": args.ratio,
                          "ms": {"multiband": plain, "seam_multiband": routed, "seam_route": alone},
                          "ratio_to_multiband": round(routed["median"] / plain["median"], 3),
                          "classes": stats[0], "rounds": stats[1], "most_rounds_in_a_class": stats[2],
                          "owner_changed": stats[3], "open_pixels": stats[4], "groups": stats[5],
                          "valid_pixels": valid}), flush=True)
        del frames, patches, table, out, argmax


if __name__ == "__main__":
    main()
