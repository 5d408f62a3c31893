"""Forged patches for the local alignment's tests (tests/test_flow_host.py,
tests/test_gpu_flow.py): the textured recipe of tests/align_cases.py (a ramp times the exponential
of block noise), random bytes, identical patches, a flat patch beside faint noise and a period-2
stripe pattern that ties every candidate - on mosaics of 130 x 257 and 67 x 300 with 3 and 4
patches whose rects are no multiples of 16 (x0 = 5 and 77) and whose widths are no multiples of 4,
with a 63-pixel intersection that is no pair, pairs of L_ij = 0, 1 and 2, masked holes inside an
overlap, three cameras on one pixel, a pair whose higher index lies first in the mosaic, alpha
quantised into ties and planted shifts out to the reach.  And the planted two-patch scenes of the
recovery and meeting tests."""
import functools

import numpy as np

import align_cases
import flow_model as fm


# ------------------------------------------------------------------------- the parts
def scene(h, w, seed, margin=40):
    """uint8 [h + 2 margin][w + 2 margin]: the textured recipe, log-encoded as a camera's tone
    curve would, so that the contrast is the same at both ends of the ramp: 40 grey levels per
    unit of log radiance around the middle of the range."""
    log = np.log(align_cases.radiance(h + 2 * margin, w + 2 * margin, seed))
    return np.clip(np.rint(128.0 + 40.0 * (log - np.median(log))), 0, 255).astype(np.uint8)


def colour_of(grey):
    """float32 [h][w][3] whose uint8(float32(255) * c) is the given byte in every plane."""
    c = ((grey.astype(np.float64) + 0.5) / 255.0).astype(np.float32)
    assert np.array_equal((np.float32(255) * c).astype(np.uint8), grey)
    return np.repeat(c[..., None], 3, axis=2)


def hat(h, w, step=None):
    """The hat weights of a frame, 0 on its border; ``step``: rounded to multiples of it."""
    y = 1.0 - np.abs(2.0 * np.arange(h) / max(h - 1, 1) - 1.0)
    x = 1.0 - np.abs(2.0 * np.arange(w) / max(w - 1, 1) - 1.0)
    a = np.outer(y, x)
    if step:
        a = np.rint(a / step) * step
    return a.astype(np.float32)


def patch(grey, y0, x0, mask=None, alpha=None, rgb=None):
    """A blender-protocol patch of grey bytes (or of uint8 [h][w][3] ``rgb``)."""
    h, w = grey.shape[:2]
    warped = np.empty((h, w, 4), np.float32)
    warped[..., :3] = colour_of(grey) if rgb is None else \
        ((rgb.astype(np.float64) + 0.5) / 255.0).astype(np.float32)
    warped[..., 3] = hat(h, w) if alpha is None else alpha
    mask = np.zeros((h, w), bool) if mask is None else mask
    return warped, mask, np.s_[y0:y0 + h, x0:x0 + w]


def cut(img, rect, shift=(0, 0), margin=40):
    """The scene as a patch at ``rect`` sees it when its content is displaced by ``shift`` =
    (dx, dy): patch[y][x] = scene[y - dy][x - dx]."""
    y0, x0, h, w = rect
    dx, dy = shift
    return img[margin + y0 - dy:margin + y0 - dy + h, margin + x0 - dx:margin + x0 - dx + w]


def holes(h, w, seed, boxes=()):
    """A mask: an invalid margin as a warp leaves it, scattered pixels, and the given boxes."""
    rng = np.random.default_rng(seed)
    m = rng.random((h, w)) < 0.01
    m[:2, :] = True
    m[:, :1] = True
    m[h - 1:, w // 2:] = True
    for y0, y1, x0, x1 in boxes:
        m[y0:y1, x0:x1] = True
    return m


# ------------------------------------------------------------------------ the GPU cases
RECTS_A = ((0, 5, 130, 150), (1, 77, 129, 179), (0, 20, 130, 201))         # on 130 x 257
RECTS_B = ((0, 5, 67, 101), (2, 43, 65, 130), (0, 77, 66, 150), (1, 150, 66, 150))  # on 67 x 300
SHAPE_A, SHAPE_B = (130, 257), (67, 300)


def _textured(rects, shape, seed, shifts, params, alpha_step=None, with_holes=True):
    img = scene(shape[0], shape[1], seed)
    out = []
    for k, (rect, shift) in enumerate(zip(rects, shifts)):
        y0, x0, h, w = rect
        mask = holes(h, w, seed + k, [(h // 3, h // 3 + 9, w // 2, w // 2 + 13)]) if with_holes else None
        out.append(patch(cut(img, rect, shift), y0, x0, mask, hat(h, w, alpha_step)))
    return out, shape, params


def _random(rects, shape, seed, params):
    rng = np.random.default_rng(seed)
    out = []
    for k, (y0, x0, h, w) in enumerate(rects):
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out.append(patch(rgb[..., 0], y0, x0, holes(h, w, seed + k), hat(h, w, 0.25), rgb=rgb))
    return out, shape, params


def _stripes(rects, shape, params):
    """Columns 40, 200, 40, 200 ... of the mosaic: dx = +-1 is the worst shift, dy ties."""
    cols = np.where(np.arange(shape[1]) % 2 == 0, 40, 200).astype(np.uint8)
    return [patch(np.repeat(cols[None, x0:x0 + w], h, 0), y0, x0) for y0, x0, h, w in rects], shape, params


def _flat(rects, shape, seed, params):
    """Patch 0 of one colour, the others 100 +- 3 of noise: no shift gains a grey level."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (y0, x0, h, w) in enumerate(rects):
        grey = np.full((h, w), 100, np.uint8) if k == 0 else \
            (100 + rng.integers(-3, 4, (h, w))).astype(np.uint8)
        out.append(patch(grey, y0, x0))
    return out, shape, params


def _identical(rects, shape, seed, params):
    img = scene(shape[0], shape[1], seed)
    return [patch(cut(img, r), r[0], r[1]) for r in rects], shape, params


@functools.lru_cache(maxsize=None)
def case(name):
    P = fm.Params
    a_swapped = (RECTS_A[1], RECTS_A[2], RECTS_A[0])
    makers = {
        # L_ij = 1, 2, 2; three cameras on the pixels of x 77 .. 155; holes in the overlaps
        "three-130x257": lambda: _textured(RECTS_A, SHAPE_A, 11, ((0, 0), (3, -2), (-2, 1)), P()),
        # the pair (0, 2) has camera 2 on the left; random bytes; alpha in steps of 1/4
        "swapped-130x257": lambda: _random(a_swapped, SHAPE_A, 12, P()),
        # L_ij = 1 everywhere, patch 0 has no pair (63 columns in common); shifts at the reach 3
        "four-67x300": lambda: _textured(RECTS_B, SHAPE_B, 13, ((0, 0), (0, 0), (3, -3), (0, 3)), P(),
                                         alpha_step=0.125),
        # ... and with pairs from 32 x 32 on the 63 columns are a pair of L_ij = 0
        "level0-67x300": lambda: _textured(RECTS_B, SHAPE_B, 14, ((0, 0), (1, 0), (-1, 1), (0, 0)),
                                           P(3, 16, 32)),
        # capped by the parameter: L_ij = 1, 1, 1, and a larger gain
        "capped-130x257": lambda: _textured(RECTS_A, SHAPE_A, 15, ((0, 0), (-3, 3), (1, 2)), P(1, 40),
                                            with_holes=False),
        "level4-130x257": lambda: _textured(RECTS_A, SHAPE_A, 16, ((0, 0), (6, -5), (-4, 7)), P(4, 16)),
        "stripes-67x300": lambda: _stripes(RECTS_B, SHAPE_B, P()),
        "flat-67x300": lambda: _flat(RECTS_B[1:], SHAPE_B, 17, P()),
        "identical-130x257": lambda: _identical(RECTS_A, SHAPE_A, 18, P()),
    }
    patches, shape, params = makers[name]()
    for warped, mask, _ in patches:
        warped.setflags(write=False)
        mask.setflags(write=False)
    return tuple(patches), shape, params


CASES = ("three-130x257", "swapped-130x257", "four-67x300", "level0-67x300", "capped-130x257",
         "level4-130x257", "stripes-67x300", "flat-67x300", "identical-130x257")
ZERO_FIELDS = ("stripes-67x300", "flat-67x300")


@functools.lru_cache(maxsize=None)
def model_of(name):
    """(aligned patches, stages) of the model on a case, made once and shared."""
    patches, shape, params = case(name)
    return fm.align(list(patches), shape, params, want_stages=True)


# ------------------------------------------------------------- recovery and meeting
# (h, w) of the two patches, which share one rect at the mosaic's origin: L_ij = 1, 2, 3.  The
# sides are a few pixels above multiples of the top level's block, 16 * 2^L, so that every block of
# every level that holds an interior level-0 block lies inside the overlap: a level-0 block whose
# ancestor straddles the overlap's border inherits from a block that sees less than the shift
# needs (on 164 x 180 at (3, 5) the model misses 12 of 90 interior blocks for every shift >= 4).
RECOVERY_SIZES = {1: (103, 107), 2: (199, 203), 3: (391, 395)}


def plants_of(level):
    r = fm.reach(level)
    half = (r + 1) // 2
    return [(0, 0), (1, 0), (0, -1), (-1, 1), (half, 0), (-half, half), (half, -1), (r, 0), (0, -r),
            (r, r), (-r, r), (r - 1, -r)]


PLANTS = tuple((level, v) for level in (1, 2, 3) for v in dict.fromkeys(plants_of(level)))
# the plants the model misses (tests/test_flow_host.py checks that these are exactly the misses)
NOT_RECOVERED = frozenset({(3, (-15, 15)), (3, (14, -15))})


@functools.lru_cache(maxsize=None)
def planted(level, vector):
    """Two patches on one rect: the scene, and the scene displaced by ``vector``."""
    h, w = RECOVERY_SIZES[level]
    img = scene(h + 8, w + 8, 100 + level)
    rect = (0, 0, h, w)
    a, b = patch(cut(img, rect), 0, 0), patch(cut(img, rect, vector), 0, 0)
    return (a, b), (h + 8, w + 8), fm.Params(level)


def interior_blocks(pair, level):
    """Boolean [nby][nbx]: the level-0 blocks wholly inside the pair's intersection and at least
    the reach from its border."""
    by0, bx0, nby, nbx = fm.block_range(pair, 0)
    _, _, _, y0, y1, x0, x1 = pair
    r = fm.reach(level)
    ys, xs = 16 * (by0 + np.arange(nby)), 16 * (bx0 + np.arange(nbx))
    return ((ys >= y0 + r) & (ys + 16 <= y1 - r))[:, None] & ((xs >= x0 + r) & (xs + 16 <= x1 - r))[None, :]
