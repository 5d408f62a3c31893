"""Write the MSOP detector's test vectors, tests/golden/msop_*.npz (CPU only).

Runs the reference's ``msop_detect`` on seeded uint8 frames and stores plain arrays: the input,
``max_feat``, the reference's points and descriptors, and per level what its ``ssc`` was handed
and what it returned.  The reference is imported from the directory given by --reference at
generation time, behind the repository's NumPy stand-in for ``cv2``; nothing of it is stored but
its outputs.  For the run the stand-in gains ``cvtColor(BGR2GRAY)``, ``Sobel``, ``cornerHarris``,
``warpPerspective`` with a constant border and ``KeyPoint``, all taken from tests/msop_model.py
(oracle/ is not edited), and the reference module sees a NumPy namespace whose ``argsort`` is
stable: the reference sorts with NumPy's default kind, which leaves the order of equal responses
open, and the stable order is one of the orders the default may return - the one this project
pins.

A case in which the reference raises or a level returns fewer than 4 points is refused.  The
model's descriptors are compared on the way: the reference inverts its float32 matrix through
LAPACK, which moves some sample coordinates across a 1/32 rounding boundary, so a few patches
differ by one tap's weight.  More than 5 % of patches differing refuses the case; the worst
difference is stored (``desc_worst``) and bounds the tests.  The files are written with fixed zip
timestamps: a rerun gives the same bytes.

    python tools/gen_msop_golden.py --reference <dir of the reference>
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (not ROOT itself: its top-level features.py shim would shadow the reference's)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import msop_model as mm  # noqa: E402
from gen_poisson_golden import save_npz  # noqa: E402

# (name, max_feat)
CASES = (("noise", (100, 50, 12, 6)),
         ("odd", (100, 50, 12, 6)),
         ("flat", (100, 50, 12, 6)))


class StableNumpy:
    """NumPy, with ``argsort`` stable unless a kind is asked for."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def argsort(a, *args, **kwargs):
        kwargs.setdefault("kind", "stable")
        return np.argsort(a, *args, **kwargs)


def install_cv2():
    """The stand-in as ``cv2``, with what ``msop_detect`` needs beyond it."""
    import cv2_shim
    cv2_shim.install()
    keep_cvt = cv2_shim.cvtColor

    def cvt_color(img, code):
        if code == cv2_shim.COLOR_BGR2GRAY:
            return mm.gray_u8(img).astype(np.uint8)
        return keep_cvt(img, code)

    def sobel(src, ddepth, dx, dy, ksize=3, scale=1.0):
        assert ddepth == cv2_shim.CV_32F and ksize == 3
        return mm.sobel(src, dx, dy, scale)

    def corner_harris(src, blockSize, ksize, k):
        assert (blockSize, ksize) == (2, 3)
        return mm.corner_harris(src, k)

    cv2_shim.cvtColor, cv2_shim.Sobel, cv2_shim.cornerHarris = cvt_color, sobel, corner_harris
    cv2_shim.warpPerspective, cv2_shim.KeyPoint = mm.warp_perspective, mm.KeyPoint
    return cv2_shim


def load_reference(directory):
    install_cv2()
    sys.path.insert(0, os.path.abspath(directory))
    ref = importlib.import_module("features")
    assert os.path.dirname(os.path.abspath(ref.__file__)) == os.path.abspath(directory)
    ref.np = StableNumpy()
    return ref


def run_reference(ref, img, max_feat):
    """(points, descs, [(ssc input, ssc output) per level]) of the reference's msop_detect."""
    calls, keep = [], ref.ssc

    def spy(keypoints, im_size, n_points, tol=0.1):
        out = keep(keypoints, im_size, n_points, tol)
        calls.append((np.array(keypoints, np.int32), np.array(out, np.int32).reshape(-1, 2)))
        return out

    ref.ssc = spy
    try:
        points, descs = ref.msop_detect(img.copy(), max_feat)
    finally:
        ref.ssc = keep
    return np.asarray(points, np.float64), np.asarray(descs, np.float32), calls


def compare_descriptors(img, max_feat, points, descs):
    """(patches that differ from the model's, worst difference), the model fed the reference's
    angles."""
    theta, start, per_level = points[:, 2].astype(np.float32), 0, []
    for lvl in range(len(max_feat)):
        n = int(np.sum(points[:, 3] == 2 ** lvl))
        per_level.append(theta[start:start + n])
        start += n
    m_points, m_descs = mm.detect(img, max_feat, thetas_in=per_level)
    assert np.array_equal(m_points, points), "the model's points differ from the reference's"
    diff = np.abs(m_descs.astype(np.float64) - descs.astype(np.float64)).max(axis=1)
    return int(np.count_nonzero(diff)), float(diff.max())


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--reference", required=True, help="directory of the reference sources")
    parser.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = parser.parse_args()
    ref = load_reference(args.reference)

    for name, max_feat in CASES:
        img = mm.fixture_image(name)
        points, descs, calls = run_reference(ref, img, max_feat)     # (a raise refuses the case)
        counts = [len(out) for _, out in calls]
        assert len(calls) == len(max_feat) and min(counts) >= 4, f"{name}: levels gave {counts}"
        m_theta = mm.detect(img, max_feat)[0][:, 2]
        assert np.array_equal(m_theta.astype(np.float32), points[:, 2].astype(np.float32)), \
            f"{name}: the model's angles differ"
        n_diff, worst = compare_descriptors(img, max_feat, points, descs)
        assert n_diff <= 0.05 * len(descs), f"{name}: {n_diff} of {len(descs)} patches differ"
        arrays = {"img": img, "max_feat": np.asarray(max_feat, np.int32), "points": points,
                  "descs": descs, "desc_worst": np.float64(worst)}
        for lvl, (given, out) in enumerate(calls):
            arrays[f"ssc_in_{lvl}"], arrays[f"ssc_out_{lvl}"] = given, out
        path = os.path.join(args.out, f"msop_{name}.npz")
        save_npz(path, arrays)
        print(f"{path}: {os.path.getsize(path)} bytes; ssc in {[len(g) for g, _ in calls]}, out "
              f"{counts}; {n_diff} of {len(descs)} patches differ from the model, worst {worst:.4g}")


if __name__ == "__main__":
    main()
