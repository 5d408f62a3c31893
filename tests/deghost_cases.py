"""Forged exposure stacks for the deghosting tests (tests/test_deghost_host.py,
tests/test_gpu_deghost.py) at the sizes of tests/align_cases.py - odd sides, widths that are no
multiple of 32, one frame beyond a tile in both directions: random bytes, identical frames, a flat
frame, a frame all 0 beside one all 255, independent 8 x 8 block noise per exposure (raw masks
with blobs that survive an erosion and cross word and tile borders), and the planted scene: a
disc that stands elsewhere in every exposure of a -/0/+ bracket."""
import functools

import numpy as np

import align_cases
import deghost_model

SIZES = align_cases.SIZES + (align_cases.BIG,)
# (slack, tol, erode, dilate): the defaults, nothing at all, the widest clean-up, each half alone,
# and every parameter at its upper end
PARAMS = ((3, 8, 1, 3), (0, 0, 0, 0), (1, 2, 3, 15), (2, 4, 0, 15), (2, 4, 3, 0), (15, 255, 3, 15))


def blocks_stack(h, w, k, seed):
    """Every exposure its own noise, constant on 8 x 8 blocks."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        coarse = rng.integers(0, 256, (-(-h // 8), -(-w // 8), 3), dtype=np.uint8)
        out.append(np.ascontiguousarray(np.repeat(np.repeat(coarse, 8, axis=0), 8, axis=1)[:h, :w]))
    return out


# ------------------------------------------------------------- the planted scene
GAINS = ((0.25, 1.0, 4.0), (0.5, 1.0, 2.0), (1.0, 1.0, 1.0))
PLANTED_SIZES = ((67, 129), (150, 270), (301, 517))
# kind: (the disc's radiance, its centre's x over w in the exposures 0, 1, 2): bright on the dark
# side of the ramp, dark on the bright side
DISCS = {"bright": (150.0, (0.10, 0.22, 0.34)), "dark": (3.0, (0.66, 0.78, 0.90))}
REFERENCE = 1


def disc_at(h, w, disc, e):
    """bool [h][w]: the disc of kind ``disc`` where it stands in exposure ``e``."""
    radius = min(h, w) // 8
    cx, cy = int(DISCS[disc][1][e] * w), h // 2
    yy, xx = np.mgrid[:h, :w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= radius ** 2


def scene(h, w, gains, disc=None, still=False):
    """Three exposures of ``align_cases.radiance(h, w, 7)`` at ``gains`` with unit noise; with
    ``disc`` the disc stands at its own place in every exposure, or, ``still``, at the
    reference's place in all three.  Grey BGR frames."""
    rad = align_cases.radiance(h, w, 7)
    rng = np.random.default_rng(h * 1000 + w)
    frames = []
    for e in range(3):
        r = rad.copy()
        if disc is not None:
            r[disc_at(h, w, disc, REFERENCE if still else e)] = DISCS[disc][0]
        frames.append(align_cases.render(r, gains[e], True, rng))
    return frames


def scenes():
    """(h, w, gains, disc) of the 18 planted scenes."""
    return [(h, w, g, d) for h, w in PLANTED_SIZES for g in GAINS for d in DISCS]


# ------------------------------------------------------------------- the GPU cases
_MAKERS = {"random": align_cases.random_stack, "identical": align_cases.identical_stack,
           "flat": align_cases.flat_stack, "extremes": align_cases.extremes_stack, "blocks": blocks_stack}


def _cases():
    """(kind, h, w, k, reference): every size with random bytes and with block noise, k = 2, 3 and 8
    and the reference first, in the middle and last in turn; the other kinds on a few sizes; the
    planted scene at its three sizes with a disc of either kind."""
    cases = []
    for i, (h, w) in enumerate(SIZES):
        k = (2, 3, 8)[i % 3]
        cases.append(("random", h, w, k, (0, k // 2, k - 1)[(i // 3 + i) % 3]))
        k = (3, 8, 2)[i % 3]
        cases.append(("blocks", h, w, k, (k - 1, 0, k // 2)[(i // 3 + i) % 3]))
    cases += [("identical", 33, 40, 3, 1), ("identical", 67, 129, 2, 0),
              ("flat", 17, 33, 2, 1), ("flat", 64, 48, 3, 0), ("flat", 150, 270, 3, 2),
              ("extremes", 16, 16, 2, 0), ("extremes", 67, 129, 3, 1), ("extremes", 33, 40, 2, 1),
              ("bright", 67, 129, 3, 1), ("dark", 150, 270, 3, 1), ("bright",) + align_cases.BIG + (3, 1),
              ("dark",) + align_cases.BIG + (3, 1)]
    return cases


CASES = _cases()
IDS = [f"{kind}-{h}x{w}-k{k}r{r}" for kind, h, w, k, r in CASES]
# the gains of the planted cases, by size
CASE_GAINS = dict(zip(PLANTED_SIZES, GAINS))


@functools.lru_cache(maxsize=None)
def stack_of(case):
    """The frames of a case (read-only arrays, made once)."""
    kind, h, w, k, _ = case
    if kind in DISCS:
        frames = scene(h, w, CASE_GAINS[(h, w)], kind)
    else:
        frames = _MAKERS[kind](h, w, k, 4000 + CASES.index(case))
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def model_of(case, params=PARAMS[0]):
    """The model's stages of a case under (slack, tol, erode, dilate), made once and shared."""
    return deghost_model.stages(stack_of(case), case[4], *params)
