"""Forged record tables for the multiband collapse (pano_multiband_compose), as host arrays.

A case is a dict:
  records   engine.PATCH_DTYPE [n]; ``planes`` / ``blurred`` hold OFFSETS in floats into the arenas
  planes    float32 arena: the records' [3][vh][vpitch] blocks, GUARD_FLOATS guard floats in front
            of, between and behind them
  blurred   float32 arena: the records' [L-1][4][ah][apitch] blocks, guarded the same way
  guards_planes / guards_blurred   the (start, stop) of every run of guard floats, in order
  owner     int16 [H][W], valid uint8 [H][W], shape (H, W), n_levels L

Colours (planes and copies) are uniform in [-0.5, 1.5], blurred alphas are drawn from ALPHAS,
``valid`` is 0 on a tenth of the pixels; nothing is NaN or infinite.  The floats of a row past the
rectangle's width (the pitch padding) and the guard floats hold GUARD.

Geometry obeys the header's "Windows" section: A inside V inside the patch, vx0 a multiple of 4,
V ending on a multiple of 4 or at the patch's end, both pitches multiples of 4."""
import functools

import numpy as np

from pano360_amd.engine import PATCH_DTYPE

SHAPE = (37, 203)               # no multiple of 4 or 64; four workgroup columns
GUARD_FLOATS = 64
GUARD = np.float32(-12345.0)
ALPHAS = np.array([0, 0, 1e-30, 0.25, 1, 3], np.float32)
LEVELS = tuple(range(1, 9))
STRIPS = ((0, 203), (5, 171), (64, 65), (130, 203), (0, 0))
MANY_LEVELS = 3
MANY_CUTS = (64, 65, 256, 300)  # one, two and four ballot masks; the plain scan

# The `overlap` geometry on SHAPE: (index, A in mosaic coordinates (row, column, ah, aw), the
# patch's margins around A (top, left, bottom, right), V's margins around A, extra floats of
# (vpitch, apitch)).  Records 0 - 3 and the 1 x 40 record 4 cover row 17, columns 70 - 109
# (m = 5); record 5 is 30 x 1 on the mosaic's last column, record 6 is 1 x 1 on its first pixel,
# and the two share index 5.  A's first / last columns fall on 0, 63, 64, 65, 127, 128 and 202,
# its first / last rows on 0, 3, 4 and 36.  Records 1, 4 and 5 have vx0 > 0 and ax0 > vx0,
# records 1 and 4 vy0 > 0 as well.
OVERLAP = (
    (0, (0, 0, 37, 128), (0, 0, 0, 2), (0, 0, 0, 2), (0, 0)),
    (1, (4, 64, 33, 139), (4, 24, 0, 0), (3, 4, 0, 0), (4, 0)),
    (2, (3, 63, 28, 66), (1, 53, 1, 31), (1, 53, 1, 1), (0, 4)),
    (3, (0, 65, 37, 63), (0, 5, 0, 32), (0, 5, 0, 32), (0, 0)),
    (4, (17, 70, 1, 40), (7, 10, 12, 30), (3, 2, 4, 10), (8, 8)),
    (5, (7, 202, 30, 1), (4, 12, 0, 0), (4, 4, 0, 0), (0, 0)),
    (5, (0, 0, 1, 1), (0, 0, 4, 6), (0, 0, 4, 6), (0, 4)),
)


def up4(v):
    return (int(v) + 3) & ~3


def make_record(index, box, pad, vpad, extra, shape):
    """One record (planes / blurred still 0) from A in mosaic coordinates and margins; every
    margin is clipped to what holds it, V's columns are rounded outwards to multiples of 4."""
    H, W = shape
    gy, gx, ah, aw = box
    y0, x0 = max(gy - pad[0], 0), max(gx - pad[1], 0)
    y1, x1 = min(gy + ah + pad[2], H), min(gx + aw + pad[3], W)
    h, w = y1 - y0, x1 - x0
    ay0, ax0 = gy - y0, gx - x0
    vy0, vx0 = max(ay0 - vpad[0], 0), max(ax0 - vpad[1], 0) & ~3
    vy1, vx1 = min(ay0 + ah + vpad[2], h), min(up4(ax0 + aw + vpad[3]), w)
    rec = np.zeros((), PATCH_DTYPE)
    for key, val in dict(y0=y0, x0=x0, h=h, w=w, vy0=vy0, vx0=vx0, vh=vy1 - vy0, vw=vx1 - vx0,
                         ay0=ay0, ax0=ax0, ah=ah, aw=aw, vpitch=up4(vx1 - vx0) + extra[0],
                         apitch=up4(aw) + extra[1], index=index).items():
        rec[key] = val
    return rec


def overlap_records(shape=SHAPE):
    """The `overlap` records, scaled from SHAPE to ``shape`` (extents of 1 stay 1)."""
    H, W = shape
    h0, w0 = SHAPE

    def span(lo, n, size, size0):
        a = lo * size // size0
        b = a + 1 if n == 1 else min(-(-(lo + n) * size // size0), size)
        return a, max(b - a, 1)

    out = []
    for index, (gy, gx, ah, aw), pad, vpad, extra in OVERLAP:
        y, hh = span(gy, ah, H, h0)
        x, ww = span(gx, aw, W, w0)
        if gx + aw == w0:
            x = W - ww                          # the mosaic's last column stays the last
        scale = lambda t: (t[0] * H // h0, t[1] * W // w0, t[2] * H // h0, t[3] * W // w0)  # noqa: E731
        out.append(make_record(index, (y, x, hh, ww), scale(pad), scale(vpad), extra, shape))
    return np.array(out, PATCH_DTYPE)


def many_records(rng, n=300, shape=SHAPE):
    """n seeded records with A of 3 x 5 to 9 x 11 anywhere on the mosaic, index = position."""
    H, W = shape
    out = []
    for i in range(n):
        ah, aw = int(rng.integers(3, 10)), int(rng.integers(5, 12))
        gy, gx = int(rng.integers(0, H - ah + 1)), int(rng.integers(0, W - aw + 1))
        pad = tuple(int(v) for v in rng.integers(0, 7, 4))
        vpad = tuple(int(v) for v in rng.integers(0, 5, 4))
        extra = (4 * int(rng.integers(0, 2)), 4 * int(rng.integers(0, 2)))
        out.append(make_record(i, (gy, gx, ah, aw), pad, vpad, extra, shape))
    return np.array(out, PATCH_DTYPE)


def colours(rng, shape):
    return (rng.random(shape, dtype=np.float32) * np.float32(2) - np.float32(0.5)).astype(np.float32)


def pack(blocks):
    """Blocks laid out back to back with GUARD_FLOATS guard floats in front of, between and
    behind them: (arena, offsets of the blocks, (start, stop) of the guard runs)."""
    total = GUARD_FLOATS + sum(b.size + GUARD_FLOATS for b in blocks)
    arena = np.full(total, GUARD, np.float32)
    offsets, guards, at = [], [(0, GUARD_FLOATS)], GUARD_FLOATS
    for b in blocks:
        arena[at:at + b.size] = b.reshape(-1)
        offsets.append(at)
        at += b.size
        guards.append((at, at + GUARD_FLOATS))
        at += GUARD_FLOATS
    assert at == total
    return arena, offsets, guards


def forge(records, n_levels, shape, seed, owner_values=None):
    """The case of ``records`` (copied) with seeded planes, copies, owner and valid."""
    rng = np.random.default_rng(seed)
    H, W = shape
    records = records.copy()
    vblocks, ablocks = [], []
    for r in records:
        v = colours(rng, (3, int(r["vh"]), int(r["vpitch"])))
        v[..., int(r["vw"]):] = GUARD
        vblocks.append(v)
        a = colours(rng, (n_levels - 1, 4, int(r["ah"]), int(r["apitch"])))
        a[:, 3] = rng.choice(ALPHAS, a[:, 3].shape)
        a[..., int(r["aw"]):] = GUARD
        ablocks.append(a)
    planes, voff, vguards = pack(vblocks)
    blurred, aoff, aguards = pack(ablocks)
    records["planes"], records["blurred"] = voff or 0, aoff or 0
    if owner_values is None:
        owner_values = np.concatenate([[-1], np.unique(records["index"])])
    owner = rng.choice(np.asarray(owner_values, np.int16), (H, W)).astype(np.int16)
    valid = (rng.random((H, W)) >= 0.1).astype(np.uint8)
    case = dict(records=records, planes=planes, blurred=blurred, guards_planes=vguards,
                guards_blurred=aguards, owner=owner, valid=valid, shape=(H, W),
                n_levels=int(n_levels))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def case(name, n_levels):
    """`overlap` (L = 2 .. 8), `one_level` (L = 1), `many` (L = MANY_LEVELS), `empty` (any L)."""
    if name == "overlap":
        assert n_levels >= 2
        return forge(overlap_records(), n_levels, SHAPE, 1000 + n_levels)
    if name == "one_level":
        assert n_levels == 1
        return forge(overlap_records(), 1, SHAPE, 1001)
    if name == "many":
        assert n_levels == MANY_LEVELS
        return forge(many_records(np.random.default_rng(77)), n_levels, SHAPE, 78)
    if name == "empty":
        return forge(np.zeros(0, PATCH_DTYPE), n_levels, SHAPE, 2000 + n_levels, owner_values=[-1, 0])
    raise KeyError(name)


RIG_LEVELS = (1, 3, 5)


@functools.lru_cache(maxsize=None)
def rig_scene():
    """The real tiny rig the interior pixels are checked on: 3 noise frames of 64 x 48, 25
    degrees apart, jitter 0.02 -> (imgs, rots, intrs, max_resolution)."""
    from pano360_amd import synth
    imgs, rots, intrs = synth.make_scene(3, 64, 48, step_deg=25.0, jitter=0.02, seed=11, kind="A")
    return imgs, rots, intrs, 400


def rig_case(shape, n_levels):
    """The `overlap` records scaled to the rig's mosaic, forged as above (the test puts the
    rig's own owner and valid maps in)."""
    return forge(overlap_records(shape), n_levels, shape, 3000 + n_levels)


def cut(case_, n):
    """The case with the first n records of its table (same arenas)."""
    out = dict(case_)
    out["records"] = case_["records"][:n]
    return out


def compose_params():
    """(name, n_levels, n or None) of every case x level the collapse is run on."""
    out = [("one_level", 1, None)] + [("overlap", lv, None) for lv in LEVELS if lv >= 2]
    out += [("many", MANY_LEVELS, n) for n in MANY_CUTS]
    out += [("empty", lv, None) for lv in LEVELS]
    return out


def param_id(p):
    name, lv, n = p
    return f"{name}-L{lv}" + (f"-n{n}" if n is not None else "")


def get(p):
    name, lv, n = p
    c = case(name, lv)
    return cut(c, n) if n is not None else c
