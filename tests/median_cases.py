"""Inputs the median blend's host and GPU tests share."""
import numpy as np


def bl_patches(g):
    out = []
    for i in range(int(g["bl_n"])):
        y0, y1, x0, x1 = (int(v) for v in g[f"bl_irange_{i}"])
        out.append((g[f"bl_warped_{i}"].copy(), g[f"bl_mask_{i}"].copy(), np.s_[y0:y1, x0:x1]))
    return out


def ghost_frames(step_deg):
    """Nine 64 x 48 frames of one smooth panorama, ``step_deg`` apart, and the same frames with a
    magenta block painted into the middle one: (rots, intrs, clean frames, painted frames)."""
    from pano360_amd import synth
    pano = synth.make_frame(7, 512, 256, "B")
    rots, intrs = synth.make_cameras(9, 64, 48, step_deg=step_deg)
    clean = [f.numpy() for f in synth.render_rig(pano, rots, intrs, 64, 48, "cpu")]
    painted = [f.copy() for f in clean]
    painted[4][16:30, 24:40] = (255, 0, 255)
    return rots, intrs, clean, painted


def ghost_rig(oracle, step_deg):
    """The oracle's patches of ``ghost_frames``: (shape, clean patches, painted patches, and what
    ``ghost_frames`` returned)."""
    rig = ghost_frames(step_deg)
    rots, intrs, clean, painted = rig
    plan, patches_clean, _ = oracle.warp_all(clean, rots, intrs, False, 1400)
    _, patches_painted, _ = oracle.warp_all(painted, rots, intrs, False, 1400)
    return plan.shape, patches_clean, patches_painted, rig


def ghost_region(shape, patches_clean, patches_painted):
    """Where the painted frame's warped colour differs from the clean one's."""
    region = np.zeros(shape, bool)
    region[patches_clean[4][2]] = (patches_clean[4][0][..., :3]
                                   != patches_painted[4][0][..., :3]).any(axis=-1)
    return region
