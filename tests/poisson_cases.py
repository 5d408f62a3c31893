"""Forged inputs of the Poisson blend (csrc/poisson.hip): masks, shapes and images chosen for
the places where its kernels take another path, for tests/test_poisson_cases_host.py (CPU) and
tests/test_gpu_poisson_forged.py (GPU).  No GPU import.

``CASES[name]`` is a ``Case(src, tgt, mask, cls)``: uint8 images ``[H][W][C]`` (C <= 4), a bool
mask ``[H][W]`` and a class,
  "generic"   the direct solve leaves at most LEFT_OUT of the mask per channel within GUARD of an
              integer, so the bytes can be compared with the reference's as the fixtures' are;
  "integral"  the mask makes the solution integral by construction - a full mask has A = P
              almost everywhere, so x = src; an isolated pixel has x = k / 4 - and a byte
              comparison is a coin toss at many pixels: the share left out is not capped, the
              bytes there are held to one level, and every byte to the truncation of the
              returned solution, which is exact for every case.  One channel above the cap
              makes a case integral.
Images are ``poisson_model.textured`` unless stated, with the seed in SEEDS; the seeds of the
generic cases were searched so that the case is within the cap (test_poisson_cases_host.py
asserts both classes).  The largest case is 67 x 131 = 8777 elements: five of the kernels'
2048-element blocks, the last one partial, and an odd width, so that a row starts on either
half of a lane's pair of elements.

``solved(name)`` is ``poisson_model.solve`` of a case, computed once per process.
"""
import functools
from collections import namedtuple

import numpy as np

import poisson_model as pm

GUARD = 1e-4                    # as tests/test_gpu_poisson.py
LEFT_OUT = 0.002

Case = namedtuple("Case", "src tgt mask cls")

BIG = (67, 131)                 # N = 8777: blocks at flat 2048, 4096, 6144, 8192
MID = (33, 47)
# single mask pixels at 67 x 131, by flat index: both halves of a lane's pair, the first and last
# elements of a wave's 128 and of a block's 2048, a pixel straight above and below a block border
# (their vertical neighbours lie in other blocks), and the last two pixels
SINGLES = (0, 1, 127, 128, 129, 2047, 2048, 2049, 4095, 4096, 2048 - 131, 2048 + 131,
           67 * 131 - 2, 67 * 131 - 1)


@functools.lru_cache(maxsize=None)
def _textured(H, W, C, seed):
    img = pm.textured(H, W, C, seed)
    img.setflags(write=False)
    return img


def _images(shape, C, seed):
    return _textured(*shape, C, seed), _textured(*shape, C, seed + 1)


def ellipse(H, W, cx=0.5, cy=0.5, rx=0.3, ry=0.3):
    """An ellipse in the interior (with the defaults it touches no border column or row)."""
    y, x = np.mgrid[:H, :W]
    return ((x - cx * W) / (rx * W)) ** 2 + ((y - cy * H) / (ry * H)) ** 2 <= 1.0


def _flat(shape, indices):
    m = np.zeros(shape[0] * shape[1], bool)
    m[list(indices)] = True
    return m.reshape(shape)


def _blobs():
    """Small blobs across the wave border 127/128 and the block borders 2047/2048, 4095/4096 and
    6143/6144, a piece in each of the first and last corners, and two pieces that the wrap link
    couples across a row end."""
    H, W = BIG
    m = np.zeros(BIG, bool)
    for i in (127, 2047, 4095, 6143):
        y, x = divmod(i, W)
        m[max(y - 1, 0):y + 2, x - 1:x + 3] = True
    m[:2, :3] = True
    m[-2:, -3:] = True
    m[20:23, -2:] = True
    m[21:24, :2] = True
    m[50, -1] = m[51, 0] = True
    return m


def _sieve():
    y, x = np.mgrid[:BIG[0], :BIG[1]]
    return ~((y % 7 == 0) & (x % 5 == 0))


def _half_and_row():
    m = np.zeros(BIG, bool)
    m[:, 65:] = True
    m[40] = True
    return m


def _wrap():
    m = np.zeros(MID, bool)
    m[10:25, -3:] = True
    m[10:25, :3] = True
    return m


def _cols(shape, *cols):
    m = np.zeros(shape, bool)
    m[:, list(cols)] = True
    return m


def _rows(shape, lo, hi):
    m = np.zeros(shape, bool)
    m[lo:hi + 1] = True
    return m


def _isolated():
    m = np.zeros(MID, bool)
    m[1:-1:2, 1:-2:2] = True
    return m


def _parity(odd):
    return (np.arange(MID[0] * MID[1]) % 2 == int(odd)).reshape(MID)


# name: (shape, channels, mask, class)
_TABLE = {
    "wrap": (MID, 3, _wrap(), "generic"),
    "col_last": (MID, 3, _cols(MID, -1), "generic"),
    "col_first": (MID, 3, _cols(MID, 0), "generic"),
    "col_w2": (BIG, 3, _cols(BIG, -2), "generic"),
    "cols_w2_w1": (BIG, 3, _cols(BIG, -2, -1), "generic"),
    "rows_9x3": ((9, 3), 3, _rows((9, 3), 2, 7), "generic"),
    "rows_7x2": ((7, 2), 3, _rows((7, 2), 1, 5), "generic"),
    "col1_7x2": ((7, 2), 3, _cols((7, 2), 1), "generic"),
    "cols_1x9": ((1, 9), 3, _cols((1, 9), 2, 3, 4, 5, 6), "generic"),
    "blobs": (BIG, 3, _blobs(), "generic"),
    "sieve": (BIG, 3, _sieve(), "generic"),
    "half_and_row": (BIG, 3, _half_and_row(), "generic"),
    "one_pixel": (MID, 3, _flat(MID, [16 * 47 + 20]), "generic"),
    "two_adjacent": (MID, 3, _flat(MID, [16 * 47 + 20, 16 * 47 + 21]), "generic"),
    "pair_over_row_end": (MID, 3, _flat(MID, [16 * 47 + 46, 17 * 47]), "generic"),
    "col0_7x2": ((7, 2), 3, _cols((7, 2), 0), "integral"),
    "row_1x300": ((1, 300), 3, _cols((1, 300), *range(40, 260)), "integral"),
    "isolated": (MID, 3, _isolated(), "integral"),
    "odd_flat": (MID, 3, _parity(True), "integral"),
    "even_flat": (MID, 3, _parity(False), "integral"),
}
for _shape in ((1, 2), (1, 3), (2, 2), (7, 2), (9, 3), (1, 300), MID, (45, 91)):
    _TABLE["full_%dx%d" % _shape] = (_shape, 3, np.ones(_shape, bool), "integral")
for _i in SINGLES:
    _TABLE["single_%d" % _i] = (BIG, 3, _flat(BIG, [_i]), "generic")

# the seed of src; tgt has seed + 1
SEEDS = {name: 100 for name in _TABLE}
SEEDS.update({"wrap": 101, "blobs": 104, "one_pixel": 102, "single_1": 102, "single_127": 101,
              "single_128": 102, "single_129": 102, "single_2047": 101, "single_2048": 104,
              "single_2049": 101, "single_8775": 101})

CLIP_SEED = 300
SAME_SEED = 310
SAME_GENERIC = (0, 2, 3)


def _clip():
    """An ellipse cut by no border; the source a random 0 / 255 checkerboard, whose Laplacian
    reaches +-1020, the target dark in channel 0 and bright in channel 1: solutions far below 0
    and far above 255."""
    H, W = 40, 52
    rng = np.random.default_rng(CLIP_SEED)
    src = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    tgt = _textured(H, W, 3, CLIP_SEED + 1).copy()
    tgt[..., 0] //= 8
    tgt[..., 1] = 255 - tgt[..., 0]
    return Case(src, tgt, ellipse(H, W, 0.55, 0.5, 0.36, 0.4), "generic")


def _same_channel():
    """Four channels; channel 1 of the source is the target's.  On an interior mask the rows of
    A and P coincide, so r0 of that channel is exactly 0: it has converged before the first
    iteration while the other three run.  Its solution is the target, all integers, which makes
    the case "integral"; SAME_GENERIC names the channels that are within the cap."""
    H, W = 40, 52
    src, tgt = _images((H, W), 4, SAME_SEED)
    src = src.copy()
    src[..., 1] = tgt[..., 1]
    return Case(src, tgt, ellipse(H, W), "integral")


def _zero():
    """b = 0: ||b|| = 0, the threshold is 0 and r0 = 0."""
    H, W = 40, 52
    z = np.zeros((H, W, 3), np.uint8)
    return Case(z, z.copy(), ellipse(H, W), "integral")


def _build():
    cases = {}
    for name, (shape, C, mask, cls) in _TABLE.items():
        src, tgt = _images(shape, C, SEEDS[name])
        cases[name] = Case(src, tgt, mask, cls)
    cases["clip"] = _clip()
    cases["same_channel"] = _same_channel()
    cases["zero"] = _zero()
    for case in cases.values():
        for a in case[:3]:
            a.setflags(write=False)
    return cases


CASES = _build()


@functools.lru_cache(maxsize=None)
def solved(name):
    """(float64 solutions [C][H][W], the reference's uint8 image) of a case, by the direct solve;
    shared by the tests and read-only."""
    case = CASES[name]
    sol, image = pm.solve(case.src, case.tgt, case.mask)
    sol.setflags(write=False)
    image.setflags(write=False)
    return sol, image


def near_integer_share(name):
    """Per channel, the share of the mask whose solution is within GUARD of an integer that a
    truncation could cross: what a byte comparison with the reference has to leave out."""
    case = CASES[name]
    sol, _ = solved(name)
    return np.array([np.mean(~pm.safe_pixels(s[case.mask], GUARD)) for s in sol])
