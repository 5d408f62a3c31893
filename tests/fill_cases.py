"""The images and masks of tests/test_gpu_fill.py, shared with tests/test_fill_host.py (which
checks, with the model, how many hole pixels of each case may round either way)."""
import functools

import numpy as np

import fill_model as fm


def noise(h, w, seed, low=0):
    return np.random.default_rng(seed).integers(low, 256, size=(h, w, 3), dtype=np.uint8)


def ramp(h, w):
    """A smooth image: three planes of different slopes."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    fy, fx = y / max(h - 1, 1), x / max(w - 1, 1)
    planes = (20 + 200 * fx + 30 * fy, 240 - 150 * fy - 60 * fx, 128 + 100 * np.sin(3 * fx + 2 * fy))
    return np.clip(np.rint(np.stack(planes, axis=-1)), 0, 255).astype(np.uint8)


def _mask(h, w, name):
    if name == "valid":
        return np.ones((h, w), np.uint8)
    if name == "invalid":
        return np.zeros((h, w), np.uint8)
    if name == "sparse":                            # small images: every third pixel or so is valid
        return (np.random.default_rng(SMALL_SEEDS[h, w][0]).random((h, w)) < 0.35).astype(np.uint8)
    mask = fm.blobs(h, w, max(4, h * w // 6000), max(3.0, min(h, w) / 7), seed=h + w)
    if name == "seam":                              # a hole across column 0, wider on the left
        mask[h // 3:h // 3 + h // 4, :w // 20 + 3] = 0
        mask[h // 3:h // 3 + h // 4, -(w // 30 + 2):] = 0
    return mask


# Means of two bytes and quarter weights put many values of a tiny image exactly on a half, where
# the comparison would allow either rounding.  (mask seed, noise seed) of the small shapes are the
# first for which the float64 model has no value near a half (tests/test_fill_host.py checks it).
SMALL_SEEDS = {(1, 7): (3, 1), (7, 1): (2, 1), (5, 9): (3, 1)}
# name -> (h, w, mask kind, closed)
SHAPES = {
    "1x1_valid": (1, 1, "valid", False),
    "1x1_invalid": (1, 1, "invalid", False),
    "1x7": (1, 7, "sparse", False),
    "7x1": (7, 1, "sparse", False),
    "5x9": (5, 9, "sparse", False),
    "64x64_tail_alone": (64, 64, "blobs", False),
    "65x64_one_pull": (65, 64, "blobs", False),
    "131x257_closed": (131, 257, "seam", True),
    "611x1103_open": (611, 1103, "blobs", False),
    "611x1103_closed": (611, 1103, "seam", True),
}
CASES = [f"{shape}-{kind}" for shape in SHAPES for kind in ("noise", "ramp")]


@functools.lru_cache(maxsize=None)
def case(name):
    """(image, mask, closed, model result, model f_0) of a case, read-only."""
    shape, kind = name.rsplit("-", 1)
    h, w, mask_kind, closed = SHAPES[shape]
    img = noise(h, w, SMALL_SEEDS.get((h, w), (0, 7 * h + w))[1]) if kind == "noise" else ramp(h, w)
    mask = _mask(h, w, mask_kind)
    want, f0 = fm.fill(img, mask, closed)
    for a in (img, mask, want, f0):
        a.setflags(write=False)
    return img, mask, closed, want, f0
