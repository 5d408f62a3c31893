"""The mosaics and views of tests/test_gpu_view.py, shared with tests/test_view_host.py (which
checks, with the model, how many pixels each comparison leaves out).  All mosaics are noise."""
import math

import numpy as np

from pano360_amd import view


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=tuple(shape) + (3,), dtype=np.uint8)


def _geometries():
    ring = 2 * math.pi / 67.3           # 67 columns close within 0.3 of a column
    fine = 2 * math.pi / 256
    tall = 2 * math.pi / 48
    return {
        # closed though 67 res0 != 2 pi: fx is stretched by 67 / 67.3
        "ring": view.MosaicGeometry((-math.pi, -16 * ring), (ring, ring), (33, 67)),
        "open": view.MosaicGeometry((-0.57, -0.4), (0.02, 0.02), (40, 57)),
        # both poles: the first and last rows are half a row away from them
        "sphere": view.MosaicGeometry((-math.pi, -math.pi / 2 + math.pi / 256),
                                      (fine, math.pi / 128), (128, 256)),
        # exactly closed, 256 rows: the two boundary rows of its own view are 0.78 % of it
        "tall": view.MosaicGeometry((-math.pi, -127.5 * 0.011), (tall, 0.011), (256, 48)),
    }


GEOMETRIES = _geometries()
MOSAIC_SEEDS = {"ring": 1, "open": 2, "sphere": 3, "tall": 4}


def mosaic(name):
    return noise(GEOMETRIES[name].shape, MOSAIC_SEEDS[name])


def _cases():
    cases = {}
    for yaw in (3.0, -3.1):             # the views straddle +-pi
        for fov in (2.0, 0.3):          # fov 0.3 magnifies: lod clamped at 0
            cases[f"ring_yaw{yaw}_fov{fov}"] = ("ring", [view.perspective(yaw, 0.0, 0.0, fov, (40, 24))])
    cases["open_partly_outside"] = ("open", [view.perspective(0.3, 0.0, 0.0, 1.0, (40, 24))])
    cases["sphere_levels"] = ("sphere", [LEVELS_VIEW])
    cases["sphere_cube"] = ("sphere", view.cube_faces(32))
    cases["sphere_equirect"] = ("sphere", [view.equirect(64)])
    cases["sphere_planet"] = ("sphere", [view.little_planet(48)])
    cases["ring_batch"] = ("ring", BATCH_VIEWS)
    cases["tall_identity"] = ("tall", [GEOMETRIES["tall"].own_view()])
    cases["tall_rolled"] = ("tall", [GEOMETRIES["tall"].own_view(ROLL)])
    return cases


LEVELS_VIEW = view.perspective(0.4, 0.7, 0.0, 1.57, (16, 16))      # crosses three or more levels
BATCH_VIEWS = [view.perspective(1.0, 0.2, 0.1, 1.2, (1, 1)), view.perspective(-2.0, -0.3, 0.0, 1.5, (65, 3)),
               view.perspective(3.0, 0.0, 0.0, 2.0, (40, 24))]
ROLL = 7
CASES = _cases()                        # name -> (geometry / mosaic name, views)
