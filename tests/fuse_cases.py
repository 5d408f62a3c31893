"""Forged exposure stacks for the fusion tests (tests/test_fuse_host.py, tests/test_gpu_fuse.py):
seeded random bytes, a gray stack, a posterised one, one with a frame all 0 and a frame all 255,
and the "window" scene - at sizes that cover every parity of every pyramid level, ``levels_for``
from 0 to 5, and one frame larger than every kernel's tile in both directions with a remainder."""
import functools

import numpy as np

# (h, w): levels_for = 0, 0, 0, 1, 1, 3, 4, 5
SIZES = ((1, 1), (2, 3), (3, 2), (4, 4), (5, 7), (17, 33), (64, 48), (67, 129))
# beyond the 32 x 8, 64 x 16 (the down kernel's source) and 64 x 4 tiles, with a remainder
BIG = (150, 270)
WINDOW = (96, 128)
GAINS = (0.25, 1.0, 4.0)


def random_stack(h, w, k, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(k)]


def gray_stack(h, w, k, seed):
    rng = np.random.default_rng(seed)
    return [np.repeat(rng.integers(0, 256, (h, w, 1), dtype=np.uint8), 3, axis=2) for _ in range(k)]


def poster_stack(h, w, k, seed):
    """Four values per channel in blocks of 5 x 3 pixels: flat regions (no contrast, the weights
    rest on the 1e-12) with sharp steps between them."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        coarse = rng.integers(0, 4, ((h + 4) // 5, (w + 2) // 3, 3)) * 85
        out.append(np.repeat(np.repeat(coarse, 5, axis=0), 3, axis=1)[:h, :w].astype(np.uint8))
    return out


def extremes_stack(h, w, k, seed):
    """Exposure 0 all 0, the last all 255, random bytes between them."""
    stack = random_stack(h, w, k, seed)
    stack[0][:] = 0
    stack[-1][:] = 255
    return stack


def window_radiance(seed=5, shape=WINDOW):
    """An interior with a window: the radiance rises 64-fold from the left edge to the right,
    with a texture and noise on it, in B, G, R."""
    h, w = shape
    rng = np.random.default_rng(seed)
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    base = 8.0 * 64.0 ** (x / (w - 1))
    texture = 1.0 + 0.25 * np.sin(0.9 * x) * np.cos(0.7 * y) + 0.05 * rng.standard_normal((h, w))
    return (base * texture)[..., None] * np.array([0.9, 1.0, 1.1])


def window_stack(seed=5, shape=WINDOW):
    """The radiance rendered at the gains 0.25, 1 and 4, rounded and clipped to 0 .. 255."""
    rad = window_radiance(seed, shape)
    return [np.clip(np.rint(rad * g), 0, 255).astype(np.uint8) for g in GAINS]


_MAKERS = {"random": random_stack, "gray": gray_stack, "poster": poster_stack, "extremes": extremes_stack}


def _cases():
    cases = []
    for i, (h, w) in enumerate(SIZES):
        cases.append(("random", h, w, (2, 3, 8)[i % 3]))
    cases += [("gray", 5, 7, 2), ("gray", 17, 33, 3), ("poster", 64, 48, 3), ("poster", 67, 129, 2),
              ("extremes", 4, 4, 2), ("extremes", 17, 33, 3), ("window",) + WINDOW + (3,),
              ("random",) + BIG + (8,), ("poster",) + BIG + (3,)]
    return cases


CASES = _cases()
IDS = [f"{kind}-{h}x{w}-k{k}" for kind, h, w, k in CASES]


@functools.lru_cache(maxsize=None)
def stack_of(case):
    """The frames of a case (read-only arrays, made once)."""
    kind, h, w, k = case
    frames = window_stack() if kind == "window" else _MAKERS[kind](h, w, k, 1000 + CASES.index(case))
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)
