"""Write the Poisson blend test vectors, tests/golden/poisson_*.npz (CPU only).

Runs the reference's ``blend.poisson_blend`` on seeded textured images and stores plain arrays:
the inputs, the mask, the uint8 result, each channel's float64 ``sol`` at the mask pixels, and
the products ``poisson_matrix(W, H) @ v`` and ``poisson_matrix(W, H, positions) @ v`` for a few
seeded vectors ``v`` of small integers (so the products are exact whatever the summation order).
The reference is imported from the directory given by --reference at generation time (with the
repository's NumPy stand-in for ``cv2``, which its imports need); nothing of it is stored but
its outputs.  ``sol`` is taken from the outside: the module's ``spsolve`` attribute is wrapped
while ``poisson_blend`` runs.

Per case and channel the share of mask pixels whose ``sol`` lies within the tests' guard band
(1e-4) of an integer is printed: those pixels are left out of the byte comparison, and a case
that comes near the tests' cap of 0.2 % wants another seed.  The files are written with fixed
zip timestamps, so a rerun reproduces them bit for bit.

    python tools/gen_poisson_golden.py --reference <dir of the reference>
"""
import argparse
import importlib
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (not ROOT itself: its top-level blend.py / stitcher.py shims would shadow the reference's)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import poisson_model as pm  # noqa: E402

GUARD = 1e-4
N_VECTORS = 2


def ellipse_cut(H, W):
    """An ellipse whose right part the image's right edge cuts off: touches columns W-2, W-1."""
    y, x = np.mgrid[:H, :W]
    return ((x - 0.72 * W) / (0.42 * W)) ** 2 + ((y - 0.5 * H) / (0.38 * H)) ** 2 <= 1.0


def corners(H, W):
    """Two components: one on the top-left corner (flat pixel 0, column 0, the first row) with a
    hole, one on the bottom-right corner (flat pixel N-1, the last row, columns W-2 and W-1)."""
    m = np.zeros((H, W), bool)
    m[:H // 2 - 3, :W // 2 - 2] = True
    m[6:14, 9:20] = False                         # the hole
    m[H // 2 + 4:, W // 2 + 5:] = True
    m[H // 2 + 4:H // 2 + 9, W - 1] = False       # a ragged right edge: W-2 without W-1
    return m


# (name, H, W, C, mask, seed)
CASES = (("ellipse128", 96, 128, 3, ellipse_cut, 101),
         ("corners", 64, 72, 4, corners, 202),
         ("ellipse260", 300, 260, 1, ellipse_cut, 303))


def save_npz(path, arrays):
    """np.savez_compressed with fixed timestamps (a rerun gives the same bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as archive:
        for key, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            archive.writestr(info, buf.getvalue())


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

    for name, H, W, C, make_mask, seed in CASES:
        src = pm.textured(H, W, C, seed)
        tgt = pm.textured(H, W, C, seed + 1)
        mask = make_mask(H, W)
        sols = []
        solve = ref.spsolve

        def spy(a, b, solve=solve):
            sols.append(np.array(solve(a, b), np.float64))
            return sols[-1]

        ref.spsolve = spy
        try:
            result = ref.poisson_blend(src.copy(), tgt.copy(), mask.astype(np.uint8) * 255)
        finally:
            ref.spsolve = solve
        assert len(sols) == C and result.dtype == np.uint8
        inside = mask.reshape(-1)
        positions = np.flatnonzero(inside)
        rng = np.random.default_rng(seed + 2)
        vectors = rng.integers(-4, 5, (N_VECTORS, H * W)).astype(np.int8)
        mat_p = ref.poisson_matrix(W, H)
        mat_a = ref.poisson_matrix(W, H, positions)
        p_v = np.stack([mat_p @ v.astype(np.float64) for v in vectors])
        a_v = np.stack([mat_a @ v.astype(np.float64) for v in vectors])
        assert np.array_equal(p_v, np.rint(p_v)) and np.array_equal(a_v, np.rint(a_v))
        path = os.path.join(args.out, f"poisson_{name}.npz")
        save_npz(path, {"src": src, "tgt": tgt, "mask": mask.astype(np.uint8) * 255,
                        "result": result, "sol": np.stack([s[inside] for s in sols]),
                        "vectors": vectors, "p_v": p_v.astype(np.int16),
                        "a_v": a_v.astype(np.int16)})
        shares = [100.0 * np.mean(~pm.safe_pixels(s[inside], GUARD)) for s in sols]
        print(path, os.path.getsize(path), "bytes;", int(inside.sum()), "mask pixels; sol",
              f"{min(s[inside].min() for s in sols):.1f} .. "
              f"{max(s[inside].max() for s in sols):.1f}; within {GUARD:g} of an integer:",
              ", ".join(f"{v:.3f} %" for v in shares))


if __name__ == "__main__":
    main()
