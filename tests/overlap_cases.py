"""Forged inputs for ``pano_overlap_stats`` (csrc/gains.hip): ``CASES`` maps a name to a ``Case`` -
frame size, block width, hat tables, 2-4 seeded noise frames and a list of (minv, i, j) pairs -
built once at import, deterministic, no frame above 48 x 640.  The groups below (``SIZES``,
``TIES``, ``HORIZON``, ``ZERO_DEN``, ``CULL`` ...) name the cases of one family; what each family
claims about its inputs is asserted on the model alone in tests/test_overlap_host.py.

The kernel's geometry the cases are placed around: a workgroup takes a tile of 64 x 16 pixels of
frame i and skips it when the denominators m6 x + m7 y + m8 of its four corner pixels share a
sign and the hull of the corners' images misses frame j by more than 2 px; the numerators enter
as x = xb + x1 with xb the start of a column block of ``bw0`` pixels.
"""
import zlib
from collections import namedtuple

import numpy as np

TILE_W, TILE_H = 64, 16

# hats: "engine" | "ones";  frames: uint8 [n][h][w][3];  pairs: ((minv float64 [9], i, j), ...)
Case = namedtuple("Case", "h w bw0 hats hat_x hat_y frames pairs")
CASES = {}


def hat(size):
    """The engine's triangular weight (``pano360_amd.engine.hat``, compared in the host test):
    0 at index 0, 0.5 in the middle."""
    centred = np.arange(size) - size / 2
    return 0.5 - np.abs(centred / size)


def warp_bw0(h, w):
    """WarpPerspectiveInvoker's column-block width for an h x w destination."""
    return min(1024 // min(16, h), w)


def _mat(rows):
    m = np.array(rows, np.float64).reshape(9)
    m.setflags(write=False)
    return m


def translation(tx, ty):
    return _mat([1, 0, tx, 0, 1, ty, 0, 0, 1])


def scaling(s, tx=0.0, ty=0.0):
    return _mat([s, 0, tx, 0, s, ty, 0, 0, 1])


IDENTITY = translation(0, 0)


def _add(name, h, w, pairs, hats, bw0=None):
    assert name not in CASES and hats in ("engine", "ones") and 2 <= h <= 48 and 2 <= w <= 640
    pairs = tuple((_mat(m), int(i), int(j)) for m, i, j in pairs)
    n = 1 + max(max(i, j) for _, i, j in pairs)
    assert 2 <= n <= 4 and pairs
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    frames.setflags(write=False)
    hat_x, hat_y = (hat(w), hat(h)) if hats == "engine" else (np.ones(w), np.ones(h))
    hat_x.setflags(write=False)
    hat_y.setflags(write=False)
    CASES[name] = Case(h, w, warp_bw0(h, w) if bw0 is None else bw0, hats, hat_x, hat_y, frames,
                       pairs)
    return name


def _both(name, h, w, pairs, bw0=None):
    return [_add(f"{name}_{hats}", h, w, pairs, hats, bw0) for hats in ("ones", "engine")]


# ------------------------------------------------------------------------------------- sizes
# below one tile, one tile, one past a tile, two tiles and one or two past; frames under 16 rows
# and frames under 64 columns have a block width other than 64
SIZE_H = (2, 3, 15, 16, 17, 33)
SIZE_W = (2, 63, 64, 65, 129, 130)
SIZES = []


def mild_perspective(h, w, sign=1.0):
    return _mat([1.03, 0.02, -0.4, -0.015, 0.98, 0.3, sign * 0.1 / w, -sign * 0.08 / h, 1])


for _h in SIZE_H:
    for _w in SIZE_W:
        SIZES += _both(f"size_{_h}x{_w}", _h, _w,
                       [(IDENTITY, 0, 1), (mild_perspective(_h, _w), 0, 2),
                        (mild_perspective(_h, _w, -1.0), 1, 2)])


# -------------------------------------------------------------------------------------- ties
# tx, ty odd multiples of 1/64: every coordinate is k + 1/2 in 1/32 px.  cvRound takes the even
# neighbour; rounding halves away from zero takes the other one where k is even for a positive
# coordinate: at every pixel for 1/64, 5/64 and -3/64 (0.5 -> 0 | 1, 2.5 -> 2 | 3, 30.5 -> 30 | 31),
# at coordinate 0 alone for -1/64 (-0.5 -> 0 | -1, the pixel leaves the frame), never for 3/64
# (1.5 -> 2 either way).  Each pair has a coordinate of the first kind.
TIE_SHIFTS = ((1, 3), (-1, -3), (3, 5), (-3, -1), (5, 1), (-3, 3))
TIES = _both("ties_17x65", 17, 65,
             [(translation(a / 64, b / 64), k % 3, (k + 1) % 3) for k, (a, b) in
              enumerate(TIE_SHIFTS)])


# ----------------------------------------------------------------------------------- horizon
# The denominator changes sign inside the frame, 17 x 130: tiles of 64, 64 and 2 columns, of 16
# rows and 1 row.  In every HORIZON_GUARDED case a tile with corner denominators of both signs
# holds counted pixels although the hull of its corners' images misses frame j by more than 2 px:
# only the sign test keeps the tile.
HORIZON_PAIRS = {
    # den = x / 50 - 1; u = 50 (4 x - 140) / (x - 50) is 140 and 430 at x = 0 and 63, 0 at x = 35
    "horizon_along_a_column": [4, 0, -140, 0, -0.3, -1, 1 / 50, 0, -1],
    # den = y / 8 - 1; v = 8 (4 y - 20) / (y - 8) is 20 and 45.7 at y = 0 and 15, 0 at y = 5
    "horizon_along_a_row": [-0.4, 0, 0, 0, 4, -20, 0, 1 / 8, -1],
    # den = x / 40 + y / 10 - 1 is negative on a triangle of tile (0, 0) and nowhere else
    "horizon_oblique_through_one_tile": [-2, -1.75, -50, 2.25, 2.5, -20, 1 / 40, 1 / 10, -1],
    # den = (x - 64) / 32 + (y - 15) / 4, all dyadic, is exactly 0 at (64, 15), a corner pixel of
    # tile (1, 0), negative at two of its other corners and positive at the last
    "horizon_through_a_tile_corner": [0, -1.5, 8, 0.5, -4, -20, 1 / 32, 1 / 4, -5.75],
}
HORIZON_CORNER_PIXEL = (64, 15)
HORIZON_GUARDED = []
for _name, _m in HORIZON_PAIRS.items():
    HORIZON_GUARDED.append(_add(_name + "_ones", 17, 130, [(_m, 0, 1), (_m, 1, 0)], "ones"))
HORIZON_GUARDED.append(_add("horizon_along_a_column_engine", 17, 130,
                            [(HORIZON_PAIRS["horizon_along_a_column"], 0, 1)], "engine"))
# negative everywhere: the negated matrix is the same map, and the cull applies with four
# negative corners (the second case, 33 x 130, keeps one tile of nine)
HORIZON_NEGATIVE = [
    _add("horizon_negative_everywhere_17x130_ones", 17, 130,
         [(-mild_perspective(17, 130), 0, 1), (mild_perspective(17, 130), 0, 1)], "ones"),
    _add("horizon_negative_everywhere_33x130_engine", 33, 130,
         [(-scaling(4.0, -256.0, -64.0), 0, 1), (scaling(4.0, -256.0, -64.0), 0, 1)], "engine")]
HORIZON = HORIZON_GUARDED + HORIZON_NEGATIVE


# -------------------------------------------------------------------------- zero denominator
# W = 0 sends the pixel to tap (0, 0) with fractions 0: it counts where hat_y[0] hat_x[0] != 0,
# which the engine's tables (0 there) never allow.  name stem -> the pixels (x, y) with den == 0,
# or None for all of them
ZERO_DEN = {}


def _zero_den(stem, h, w, minv, pixels):
    for name in _both(stem, h, w, [(minv, 0, 1), (minv, 1, 1)]):
        ZERO_DEN[name] = pixels
    return minv


# integer m6, m7, m8: the denominators x - 5 and x + 1000 y - 9070 are exact
_zero_den("zero_den_on_column_5", 17, 65, [2, 0, 7, 0, 3, 9, 1, 0, -5],
          [(5, y) for y in range(17)])
_zero_den("zero_den_at_pixel_70_9", 17, 130, [2, 0, 7, 0, 3, 9, 1, 1000, -9070], [(70, 9)])
_zero_den("zero_den_singular_all_zero", 17, 65, np.zeros(9), None)


# -------------------------------------------------------------------------------- cull edges
# Translations that step frame j's footprint across one side of a tile in steps of 1/128 px,
# 33 x 130, all-ones tables.  Low side: the largest coordinate of tile column 0 (x = 63), or of
# tile row 0 (y = 15), runs from -1/32 to +1/32; -1/64 is the lowest coordinate that still rounds
# to tap 0.  High side: the smallest coordinate of tile column 1 (x = 64), or of tile row 1
# (y = 16), runs from w - 1 - 1/32 to w - 1 + 1/32 (h - 1 in y); a tap must be below w - 1.
CULL_H, CULL_W = 33, 130
CULL_STEPS = tuple(range(-4, 5))                  # in 1/128 px
CULL_LOW = {"cull_low_x": (0, 0), "cull_low_y": (0, 0)}          # name -> the stepped tile
CULL_HIGH = {"cull_high_x": (1, 0), "cull_high_y": (0, 1)}
_add("cull_low_x", CULL_H, CULL_W,
     [(translation(-63 + s / 128, 0), 0, 1) for s in CULL_STEPS], "ones")
_add("cull_low_y", CULL_H, CULL_W,
     [(translation(0, -15 + s / 128), 0, 1) for s in CULL_STEPS], "ones")
_add("cull_high_x", CULL_H, CULL_W,
     [(translation(CULL_W - 1 - 64 + s / 128, 0), 0, 1) for s in CULL_STEPS], "ones")
_add("cull_high_y", CULL_H, CULL_W,
     [(translation(0, CULL_H - 1 - 16 + s / 128), 0, 1) for s in CULL_STEPS], "ones")
# the footprint far off: every tile skipped; far off except for tile (1, 1), whose pixel (64, 16)
# maps to (0, 0) while every other tile maps at least 4 px outside
CULL_ALL = _add("cull_every_tile", CULL_H, CULL_W,
                [(translation(1000, 0), 0, 1), (translation(0, -1000), 1, 0),
                 (translation(-1e9, 1e9), 0, 1)], "ones")
CULL_ALL_BUT_ONE = _add("cull_every_tile_but_one", CULL_H, CULL_W,
                        [(scaling(4.0, -256.0, -64.0), 0, 1)], "ones")
CULL = list(CULL_LOW) + list(CULL_HIGH) + [CULL_ALL, CULL_ALL_BUT_ONE]


# ----------------------------------------------------------------------------- magnification
# 1e6 and 1e12: the fixed-point coordinate leaves the int32 range and is clamped, the tap leaves
# the int16 range and is saturated; 65537 and the shift by -65536: a tap cut to 16 bits instead of
# saturated would land inside the frame.  The minification maps all of frame i into texel (5, 3).
MAGNIFY = []
for _s, _tag in ((1 / 3, "one_third"), (3.0, "3"), (1e6, "1e6"), (1e12, "1e12"),
                 (65537.0, "65537")):
    MAGNIFY += _both(f"magnify_{_tag}", 17, 130, [(scaling(_s), 0, 1), (scaling(_s, 0.7, 0.4), 1, 0),
                                                  (scaling(-_s, 128.0, 16.0), 0, 1)])
MAGNIFY += _both("magnify_shift_by_65536", 17, 65, [(translation(-65536, 0), 0, 1),
                                                    (translation(0, 65536), 0, 1)])
MINIFY_TEXEL = (5, 3)
MAGNIFY += _both("minify_into_one_texel", 17, 65, [(scaling(1 / 1024, 5.3, 3.4), 0, 1)])


# ------------------------------------------------------------------------------- block width
# A perspective matrix with non-dyadic entries whose m2 is then moved, ulp by ulp, until the
# coordinate of one chosen pixel sits on a rounding boundary that the split x = xb + x1 decides:
# computed with xb = x, x1 = 0, and with xb = 0, x1 = x (one block as wide as the frame), the same
# pixel gets the neighbouring fixed-point coordinate.  The seeds are the first of 0, 1, 2 ... whose
# pixel maps inside the frame and for which the scan of +-200 ulps finds such an m2.
def _coord_at(m, k, x, y, bw0, split):
    """32 u (k = 0) or 32 v (k = 3) of pixel (x, y) before rounding, and its denominator."""
    xb, x1 = (float(x // bw0 * bw0), float(x % bw0)) if split else (float(x), 0.0)
    den = ((m[6] * xb + m[7] * y) + m[8]) + m[6] * x1
    return (((m[k] * xb + m[k + 1] * y) + m[k + 2]) + m[k] * x1) * (32.0 / den), den


def blockwidth_matrix(seed, h, w):
    """(minv, (x, y)), or None where the chosen pixel maps outside the frame or the scan fails."""
    rng = np.random.default_rng(9000 + seed)
    bw0 = 1024 // h
    m = np.array([rng.uniform(0.8, 0.95), rng.uniform(-0.02, 0.02), rng.uniform(1.0, 3.0),
                  rng.uniform(-0.02, 0.02), rng.uniform(0.8, 0.95), rng.uniform(0.2, 0.8),
                  rng.uniform(-0.1, 0.1) / w, rng.uniform(-0.1, 0.1) / h, 1.0])
    x = int(rng.integers(bw0 + 1, w - 8))
    x += x % bw0 == 0
    y = int(rng.integers(2, h - 2))
    have, den = _coord_at(m, 0, x, y, bw0, True)
    if not (64 <= have < 32 * (w - 3) and 64 <= _coord_at(m, 3, x, y, bw0, True)[0] < 32 * (h - 3)):
        return None
    m[2] += (np.floor(have) + 0.5 - have) * den / 32.0
    start = m[2]
    for direction in (np.inf, -np.inf):
        m[2] = start
        for _ in range(200):
            have = np.rint(_coord_at(m, 0, x, y, bw0, True)[0])
            if have != np.rint(_coord_at(m, 0, x, y, bw0, False)[0]) and \
                    have != np.rint(_coord_at(m, 0, x, y, w, True)[0]):
                return _mat(m), (x, y)
            m[2] = np.nextafter(m[2], direction)
    return None


BLOCKWIDTH_SHAPES = ((13, 600), (9, 640), (15, 200), (11, 333))
BLOCKWIDTH, BLOCKWIDTH_VARIANTS = {}, []           # name -> the pixel whose coordinate the split decides
_seed = 0
for _h, _w in BLOCKWIDTH_SHAPES:
    while True:
        _found = blockwidth_matrix(_seed, _h, _w)
        _seed += 1
        if _found is not None:
            break
    _stem = f"blockwidth_seed{_seed - 1}_{_h}x{_w}"
    BLOCKWIDTH[_add(_stem, _h, _w, [(_found[0], 0, 1)], "engine")] = _found[1]
    BLOCKWIDTH_VARIANTS.append(_add(_stem + "_bw64", _h, _w, [(_found[0], 0, 1)], "engine", bw0=64))
    BLOCKWIDTH_VARIANTS.append(_add(_stem + "_bw_w", _h, _w, [(_found[0], 0, 1)], "engine", bw0=_w))


# ------------------------------------------------------------------------------------ random
N_RANDOM = 60
RANDOM = []


def random_matrix(seed, h, w):
    """Seed % 3 == 0: a rotation about a point of the frame; 1: an affine map; 2: a perspective map
    with |m6|, |m7| up to 1 / w."""
    rng = np.random.default_rng(7000 + seed)
    cx, cy = rng.uniform(0, w), rng.uniform(0, h)
    if seed % 3 == 0:
        a = rng.uniform(-np.pi, np.pi)
        lin = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    else:
        lin = np.eye(2) + rng.uniform(-0.4, 0.4, (2, 2))
    shift = np.array([cx, cy]) - lin.dot([cx, cy]) + rng.uniform(-0.2, 0.2, 2) * (w, h)
    m = np.array([[lin[0, 0], lin[0, 1], shift[0]], [lin[1, 0], lin[1, 1], shift[1]], [0, 0, 1.0]])
    if seed % 3 == 2:
        m[2, :2] = rng.uniform(-1, 1, 2) / w
    return _mat(m)


for _s in range(N_RANDOM):
    _rng = np.random.default_rng(6000 + _s)
    _h, _w = int(_rng.choice(SIZE_H[2:])), int(_rng.choice(SIZE_W[1:]))
    RANDOM.append(_add(f"random_{_s:02d}_{_h}x{_w}", _h, _w,
                       [(random_matrix(_s, _h, _w), 0, 1), (random_matrix(_s + 100, _h, _w), 1, 0)],
                       "engine"))
