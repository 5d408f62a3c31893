"""Write the seam finder's test vectors, tests/golden/graph_cut_*.npz (CPU only).

Runs the reference's ``blend.graph_cut`` on seeded image pairs and stores plain arrays: the two
inputs (as uint8, with the dtype they are handed over in named beside them), ``shrink``, the
reference's label grid and its uint8 mask.  The reference is imported from the directory given by
--reference at generation time, behind the repository's NumPy stand-in for ``cv2``; nothing of it
is stored but its outputs.  That stand-in's ``resize`` restates the 8-bit call of the CLI only, so
for the run ``cv2.resize`` is tests/graph_cut_model.py's float32 restatement, and through it the
grid the reference hands over is recorded as well: ``(mask == -1)`` as float32, which *is* the
reference's label map, untouched by any restatement of ours.

Per case the share of each label and the number of classes (level, colour) that labelled a cell
are printed; a case in which a label holds less than 10 % of the grid or fewer than 20 classes
did work is refused (a degenerate seam proves nothing; ``shrink14``, the all-(+1) grid, is exempt
by name).  The sweep and the heap restatements of the model are compared with the recorded grid
on the way.  The files are written with fixed zip timestamps: a rerun gives the same bytes.

    python tools/gen_graph_cut_golden.py --reference <dir of the reference>
"""
import argparse
import importlib
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (not ROOT itself: its top-level blend.py / stitcher.py shims would shadow the reference's)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import graph_cut_model as gm  # noqa: E402
from gen_poisson_golden import save_npz  # noqa: E402


def _smooth(h, w, c, seed, dtype):
    return gm.smooth_pair(h, w, c, seed, dtype)


def _alpha(h, w, c, seed, dtype):
    return gm.with_alpha_holes(gm.smooth_pair(h, w, c - 1, seed, dtype), seed + 1)


def _noise(h, w, c, seed, dtype):
    return gm.noise_pair(h, w, c, seed, dtype)


def _islands(h, w, c, seed, dtype):
    return gm.island_pair(h, w, c, seed, dtype)


# (name, H, W, C, dtype, shrink, maker, seed)
CASES = (("smooth", 300, 260, 3, np.int16, 5, _smooth, 11),
         ("alpha", 120, 168, 4, np.float32, 2, _alpha, 22),
         ("noise", 96, 128, 3, np.int16, 1, _noise, 33),
         ("islands", 100, 150, 3, np.int16, 1, _islands, 44),
         ("odd", 203, 157, 3, np.int32, 3, _smooth, 55),
         ("shrink14", 60, 90, 3, np.int16, 14, _smooth, 66),
         ("uint8", 120, 150, 3, np.uint8, 2, _smooth, 77))


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reference", required=True, help="directory of the reference sources")
    parser.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = parser.parse_args()
    import cv2_shim
    cv2_shim.install()
    sys.path.insert(0, os.path.abspath(args.reference))
    ref = importlib.import_module("blend")
    assert os.path.dirname(os.path.abspath(ref.__file__)) == os.path.abspath(args.reference)

    for name, H, W, C, dtype, shrink, maker, seed in CASES:
        img1, img2 = maker(H, W, C, seed, dtype)
        handed = []

        def spy(src, dsize):
            handed.append(np.array(src))
            return gm.resize_f32(src, dsize)

        keep = getattr(cv2_shim, "resize")
        cv2_shim.resize = spy
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)   # uint8: the reference's wraps
                mask = ref.graph_cut(img1.copy(), img2.copy(), shrink)
        finally:
            cv2_shim.resize = keep
        assert len(handed) == 1 and handed[0].dtype == np.float32
        assert mask.dtype == np.uint8 and mask.shape == (H, W, 1)
        # the handed-over grid marks the -1 cells; every other cell is +1 once the heap is empty
        labels = np.where(handed[0] == 1.0, -1, 1).astype(np.int8)
        level = gm.levels(img1, img2, shrink)
        border = gm.border_of(shrink)
        if border == 1:
            worked = 0
            assert (labels == 1).all() and not mask.any()
        else:
            sweep, worked = gm.flood_sweep(level, border, want_stats=True)
            assert np.array_equal(sweep, labels), f"{name}: the class sweep differs"
            assert np.array_equal(gm.flood_heap(level, border), labels), f"{name}: heap differs"
        assert np.array_equal(gm.mask_from_labels(labels, H, W), mask)
        share = [float(np.mean(labels == c)) for c in (-1, 1)]
        path = os.path.join(args.out, f"graph_cut_{name}.npz")
        print(f"{path}: grid {labels.shape}, border {border}, levels {level.min()} .. "
              f"{level.max()} ({len(np.unique(level))} distinct), share of -1 {share[0]:.3f}, of +1 "
              f"{share[1]:.3f}, classes that worked {worked}")
        if name != "shrink14":
            assert min(share) >= 0.10 and worked >= 20, f"{name}: a degenerate seam"
        for img in (img1, img2):
            assert np.array_equal(img, img.astype(np.uint8).astype(dtype))
        save_npz(path, {"img1": img1.astype(np.uint8), "img2": img2.astype(np.uint8),
                        "dtype": np.array(np.dtype(dtype).name), "shrink": np.int32(shrink),
                        "labels": labels, "mask": mask})
        print("   ", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
