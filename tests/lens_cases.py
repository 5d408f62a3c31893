"""The frames and calibrations of tests/test_gpu_lens.py, shared with tests/test_lens_host.py
(which checks, with the model alone, how few pixels of each case lie near a quantisation tie).
Frames are noise or a hard checkerboard: a smooth image hides a wrong tap."""
import functools

import numpy as np

import lens_model as lm


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def checkerboard(h, w, square=5):
    """Squares of 0 and 255 (the channels' boards shifted against each other): the cubic
    weights overshoot on every edge, so the clamp to 0 .. 255 is exercised."""
    y, x = np.mgrid[0:h, 0:w]
    planes = [(((y + s) // square + (x + 2 * s) // square) & 1) * 255 for s in (0, 1, 3)]
    return np.stack(planes, axis=-1).astype(np.uint8)


# name -> (kind, fx, fy, cx, cy, k, (w, h), focal, image): focal None = the fitted one, a float = an
# override, ("fit", s) = s times the fitted one
CASES = {
    "barrel": ("brown", 100.0, 101.0, 66.3, 47.1, (-0.25, 0.05, 1e-3, -5e-4, 0.0), (131, 97), None,
               "noise"),
    "pincushion": ("brown", 100.0, 100.0, 65.5, 48.5, (0.12,), (131, 97), None, "checker"),
    "fisheye": ("fisheye", 50.0, 50.0, 80.2, 59.7, (0.02, -0.003, 0.0, 0.0), (160, 120), None,
                "noise"),
    # a tile's tail (33 = 8 threads of four pixels and one of one), fewer rows than a tile
    "33x9": ("brown", 30.0, 31.0, 16.2, 4.3, (-0.1, 0.01, 2e-3, 1e-3, 0.0), (33, 9), None, "noise"),
    # smaller than the cubic footprint: every tap is the one pixel
    "1x1": ("brown", 10.0, 10.0, 0.3, 0.2, (0.1,), (1, 1), 10.0, "noise"),
    # four pixels wide: a thread's four pixels are the row, one column position is off the border
    "4wide": ("brown", 20.0, 20.0, 1.7, 10.4, (-0.2,), (4, 21), 20.0, "checker"),
    "identity": ("brown", 40.0, 40.0, 35.0, 25.0, (), (70, 50), 40.0, "noise"),
    # 0.6 x the fitted focal length: positions leave the frame on all four sides
    "clamp": ("brown", 100.0, 101.0, 66.3, 47.1, (-0.25, 0.05, 1e-3, -5e-4, 0.0), (131, 97),
              ("fit", 0.6), "checker"),
    "fisheye_clamp": ("fisheye", 50.0, 50.0, 80.2, 59.7, (0.02, -0.003, 0.0, 0.0), (160, 120),
                      ("fit", 0.6), "checker"),
}
FITTED = ("barrel", "pincushion", "fisheye")            # the focal lengths the issue states
STATED_FOCALS = {"barrel": 97.763, "pincushion": 106.967, "fisheye": 25.627}
INTERPS = ("cubic", "linear")


@functools.lru_cache(maxsize=None)
def focal(name):
    """The case's focal length, from the model's own bisection (not from pano360_amd.lens)."""
    kind, fx, fy, cx, cy, k, size, spec, _ = CASES[name]
    if isinstance(spec, float):
        return spec
    fitted = lm.smallest_focal(kind, fx, fy, cx, cy, k, size)
    return fitted if spec is None else spec[1] * fitted


@functools.lru_cache(maxsize=None)
def image(name):
    (w, h), kind = CASES[name][6], CASES[name][8]
    img = noise(h, w, 11 * h + w) if kind == "noise" else checkerboard(h, w)
    img.setflags(write=False)
    return img


def lens_model(name):
    """The case's ``pano360_amd.lens.LensModel``."""
    from pano360_amd import lens
    kind, fx, fy, cx, cy, k, size = CASES[name][:7]
    return lens.LensModel(kind, fx, fy, cx, cy, k, size)


@functools.lru_cache(maxsize=None)
def expected(name, interp):
    """(the model's corrected frame, its near-tie mask), read-only."""
    kind, fx, fy, cx, cy, k = CASES[name][:6]
    want, near = lm.undistort(image(name), kind, fx, fy, cx, cy, k, focal(name), interp)
    want.setflags(write=False)
    near.setflags(write=False)
    return want, near
