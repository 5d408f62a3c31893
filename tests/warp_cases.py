"""Rigs and forged window tables for the window warp (pano_warp_windows), as host data.

All frames are seeded noise; the mosaics are capped to a few hundred columns.  A rig is a dict of
imgs (uint8 frames), rots, intrs, max_resolution and ``stretch`` (every patch rectangle is
replaced by the whole mosaic, so that each patch sees the back hemisphere)."""
import functools

import numpy as np

from pano360_amd import synth
from pano360_amd.bundle_adj import intrinsics, rotation_to_mat
from pano360_amd.engine import PATCH_DTYPE

RIGS = ("sweep", "rolled", "mixed", "behind")
GUARD_FLOATS = 64
NAN_BITS = 0x7FC5A5A5           # a quiet NaN nothing computes: "not written"
WINDOW_ROWS = (1, 3, 4, 15, 16, 17, 33)
WINDOW_X0 = (0, 4, 60, 64)
WINDOW_COLS = (4, 60, 64, 68, None)             # None: to the patch's end
MIXED_SIZES = ((1, 1), (1, 9), (7, 1), (48, 64), (2, 2), (33, 130))     # (h, w); the middle
#                                                frame, which sets the resolution, is a usual one


def _camera(yaw, pitch=0.0, roll=0.0):
    """Yaw about y, then pitch about x, then roll about the optical axis."""
    return (rotation_to_mat([0.0, 0.0, roll]).dot(rotation_to_mat([pitch, 0.0, 0.0]))
            .dot(rotation_to_mat([0.0, yaw, 0.0])))


@functools.lru_cache(maxsize=None)
def rig(name):
    if name == "sweep":
        imgs, rots, intrs = synth.make_scene(3, 64, 48, step_deg=25.0, jitter=0.05, seed=21, kind="A")
        return dict(imgs=imgs, rots=rots, intrs=intrs, max_resolution=300, stretch=False)
    if name == "rolled":
        f = synth.focal_for(64)
        # (yaw, pitch, roll, principal point); the middle frame, which sets the resolution, is level
        poses = ((-0.35, 0.5, np.pi / 2, (3, -2)), (0.0, -0.5, np.pi, (-5, 4)),
                 (0.35, 0.0, 0.0, (0, 0)), (0.7, 0.0, 0.0, (0, 0)))
        rots = np.stack([_camera(yaw, pitch, roll) for yaw, pitch, roll, _ in poses])
        intrs = np.stack([intrinsics(f, c).astype(np.float64) for *_, c in poses])
        imgs = [synth.make_frame(31 + i, 64, 48, "A") for i in range(4)]
        return dict(imgs=imgs, rots=rots, intrs=intrs, max_resolution=300, stretch=False)
    if name == "mixed":
        n = len(MIXED_SIZES)
        rots = np.stack([_camera(np.deg2rad(12.0) * (i - n // 2)) for i in range(n)])
        intrs = np.stack([intrinsics(synth.focal_for(64)).astype(np.float64)] * n)
        imgs = [synth.make_frame(41 + i, w, h, "A") for i, (h, w) in enumerate(MIXED_SIZES)]
        return dict(imgs=imgs, rots=rots, intrs=intrs, max_resolution=300, stretch=False)
    if name == "behind":
        imgs, rots, intrs = synth.make_scene(3, 64, 48, step_deg=110.0, seed=3, kind="A")
        return dict(imgs=imgs, rots=rots, intrs=intrs, max_resolution=400, stretch=True)
    raise KeyError(name)


def make_plan(plan_class, r):
    """``engine.Plan`` or the oracle's ``Plan`` of a rig (the two derive the same geometry)."""
    shapes = [im.shape[:2] for im in r["imgs"]]
    plan = plan_class(shapes, r["rots"], r["intrs"], True, r["max_resolution"])
    # where the middle of each frame lands, in mosaic coordinates (row, column)
    plan.centres = [((y0 + y1) // 2, (x0 + x1) // 2) for y0, y1, x0, x1 in plan.rects]
    if r["stretch"]:
        plan.rects = [(0, plan.shape[0], 0, plan.shape[1])] * len(shapes)
    return plan


def up4(v):
    return (int(v) + 3) & ~3


def taps_inside(mx, my, sw, sh):
    """bool per pixel of an inverse map: the four bilinear taps of cv2.remap's fixed-point
    position (5 fractional bits, int16 saturation) lie in the frame, so no border rule applies."""
    def base(m):
        s = np.rint(m * np.float32(32))
        s = np.where(np.abs(s) < 2.0 ** 31, s, -2.0 ** 31).astype(np.int64)     # NaN, inf: far outside
        return np.clip(s >> 5, -32768, 32767)
    x0, y0 = base(mx), base(my)
    return (x0 >= 0) & (x0 < sw - 1) & (y0 >= 0) & (y0 < sh - 1)


def windows_by_taps(records, maps, shapes):
    """(windows whose every pixel has its four taps in the frame - whatever the shape of a wave,
    all their waves take the path without border rule; windows with pixels of both kinds - some
    wave holds lanes inside and outside).  ``maps``: per camera the whole-patch (map_x, map_y);
    frames too small to hold four taps must have no pixel inside."""
    whole = mixed = 0
    for r in records:
        i = int(r["index"])
        sh, sw = shapes[i]
        vy0, vx0, vh, vw = (int(r[k]) for k in ("vy0", "vx0", "vh", "vw"))
        inside = taps_inside(maps[i][0], maps[i][1], sw, sh)[vy0:vy0 + vh, vx0:vx0 + vw]
        assert inside.shape == (vh, vw)
        assert min(sh, sw) > 1 or not inside.any()
        whole += bool(inside.all())
        mixed += bool(inside.any() and not inside.all())
    return whole, mixed


def _record(index, rect, window, rng):
    y0, y1, x0, x1 = rect
    vy0, vx0, vh, vw = window
    h, w = y1 - y0, x1 - x0
    assert 0 <= vy0 and vy0 + vh <= h and 0 <= vx0 and vx0 + vw <= w and vh > 0 and vw > 0
    assert vx0 % 4 == 0 and ((vx0 + vw) % 4 == 0 or vx0 + vw == w)
    # rectangle A (it only places the tile grid of the need flags): V, a little smaller
    top, bottom = (int(v) for v in rng.integers(0, 3, 2))
    left, right = (int(v) for v in rng.integers(0, 6, 2))
    ay0, ay1 = vy0 + top, vy0 + vh - bottom
    ax0, ax1 = vx0 + left, vx0 + vw - right
    if ay1 <= ay0:
        ay0, ay1 = vy0, vy0 + vh
    if ax1 <= ax0:
        ax0, ax1 = vx0, vx0 + vw
    rec = np.zeros((), PATCH_DTYPE)
    for key, val in dict(y0=y0, x0=x0, h=h, w=w, vy0=vy0, vx0=vx0, vh=vh, vw=vw, ay0=ay0, ax0=ax0,
                         ah=ay1 - ay0, aw=ax1 - ax0, vpitch=up4(vw) + 4 * int(rng.integers(0, 2)),
                         apitch=up4(ax1 - ax0), index=index).items():
        rec[key] = val
    return rec


def _window(h, w, vh, vx0, vw, corner):
    """Window of about vh x vw on corner (bottom, right) of an h x w patch, by the rules."""
    vh = min(vh, h)
    vy0 = h - vh if corner[0] else 0
    if corner[1]:                               # reaches the patch's last column
        vx0 = max(w - (vw or w), 0) & ~3
        return vy0, vx0, vh, w - vx0
    vx0 = vx0 if vx0 < w else 0
    vw = w - vx0 if vw is None or vx0 + vw > w else vw
    return vy0, vx0, vh, vw


def windows(rects, centres, seed):
    """The forged table of a rig: per patch the whole patch and three windows - two on
    opposite corners of the patch's rectangle (the pairs alternate from patch to patch) and,
    on even patches, one anywhere, on odd patches one 4 columns wide around ``centres[i]`` (the
    middle of the frame: every lane of its waves lies inside the frame) - in shuffled order.
    ``planes`` holds OFFSETS in floats into an arena with GUARD_FLOATS floats in front of,
    between and behind the blocks; returns (records, floats)."""
    rng = np.random.default_rng(seed)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]      # noqa: E731
    out = []
    for i, rect in enumerate(rects):
        h, w = rect[1] - rect[0], rect[3] - rect[2]
        out.append(_record(i, rect, (0, 0, h, w), rng))
        corners = ((0, 0), (1, 1)) if i % 2 == 0 else ((0, 1), (1, 0))
        for corner in corners:
            out.append(_record(i, rect, _window(h, w, pick(WINDOW_ROWS), pick(WINDOW_X0),
                                                pick(WINDOW_COLS), corner), rng))
        vy0, vx0, vh, vw = _window(h, w, pick(WINDOW_ROWS), pick(WINDOW_X0), pick(WINDOW_COLS), (0, 0))
        vy0 = int(rng.integers(0, h - vh + 1))
        if i % 2 and w >= 8:
            cy, cx = centres[i][0] - rect[0], centres[i][1] - rect[2]
            vy0, vx0, vw = min(max(cy - vh // 2, 0), h - vh), min(max(cx - 2, 0) & ~3, (w - 4) & ~3), 4
        out.append(_record(i, rect, (vy0, vx0, vh, vw), rng))
    rec = np.array(out, PATCH_DTYPE)[rng.permutation(len(out))]
    at = GUARD_FLOATS
    for r in rec:
        r["planes"] = at
        at += 3 * int(r["vh"]) * int(r["vpitch"]) + GUARD_FLOATS
    return rec, at
