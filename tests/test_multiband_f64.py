"""CPU: the float64 restatement of the multiband blend (tests/multiband_f64.py) checked as a
yardstick - its blur against a direct tap loop and against planes recorded while the reference
ran, its mosaic against the reference's golden mosaics, and the float32 oracle within the derived
bound E of it."""
import numpy as np
import pytest

import multiband_f64 as mf
from conftest import SCENES, load_golden, scene_inputs


def _reflect101(p, n):
    """OpenCV's borderInterpolate for BORDER_REFLECT_101, reflections repeated until in range."""
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def _blur_loop(plane, sigma):
    t = mf.level_taps(sigma)
    r = len(t) // 2
    h, w = plane.shape[:2]
    x = np.asarray(plane, np.float64)
    cols = np.array([[_reflect101(c + j - r, w) for j in range(len(t))] for c in range(w)])
    rows = np.array([[_reflect101(y + j - r, h) for j in range(len(t))] for y in range(h)])
    mid = np.einsum("j,yxj...->yx...", t, x[:, cols])
    return np.einsum("j,yjx...->yx...", t, mid[rows])


@pytest.mark.parametrize("shape", [(37, 53), (1, 40), (40, 1), (2, 45), (45, 2), (3, 3), (1, 1),
                                   (3, 70), (33, 31)])
@pytest.mark.parametrize("sigma", [4.0, 4.0 * np.sqrt(13.0)])
def test_blur_f64_equals_a_direct_tap_loop(shape, sigma):
    """Ragged planes and planes 1, 2 and 3 pixels wide or high, where REFLECT_101 bounces more than
    once (radius 16 and 58): SciPy's mirror mode is OpenCV's border, to float64 rounding."""
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    plane = rng.random(shape + (2,)).astype(np.float32)
    want = _blur_loop(plane, sigma)
    got = mf.blur_f64(plane, sigma)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)


def test_blur_f64_against_the_reference_planes():
    """The planes a spying cv2.GaussianBlur recorded inside the reference's multiband_blend (all
    four levels of one patch of the small noise scene): float32 results of the same taps, within
    the bound the analysis gives a float32 blur."""
    g = load_golden("scene_small_noise")
    worst = 0.0
    for k, sigma in enumerate(g["blur_sigma"]):
        truth = mf.blur_f64(g["blur_in"], float(sigma))
        ntaps = len(mf.level_taps(float(sigma)))
        e = mf.plane_error(g[f"blur_out_{k}"], truth, ntaps)
        worst = max(worst, float(e.max()))
        assert e.max() <= mf.plane_bound(ntaps), (k, float(e.max()))
        assert np.abs(g[f"blur_out_{k}"] - truth).max() <= 1e-6
    print(f"reference planes against the float64 blur: worst e {worst:.2f}")


@pytest.mark.parametrize("name", SCENES)
def test_multiband_f64_against_the_reference_mosaics(oracle, name):
    """The truth quantised as stitcher.py:241 does is the reference's mosaic within one level (the
    reference computes in float32), at five levels and at six where the golden holds it."""
    g = load_golden(name)
    imgs, rots, intrs, mr = scene_inputs(g)
    levels_held = [lv for lv in (5, 6) if f"mb{lv}_mosaic" in g]
    assert 5 in levels_held
    for levels in levels_held:
        plan, patches, _ = oracle.warp_all(imgs, rots, intrs, True, mr)
        truth, _, _ = mf.multiband_f64(patches, plan.shape, levels)
        want = g[f"mb{levels}_mosaic"]
        got = (255.0 * truth.astype(np.float32)).astype(np.uint8)
        assert got.shape == want.shape
        diff = np.abs(got.astype(int) - want.astype(int))
        assert diff.max() <= 1, (name, levels, int(diff.max()))
        assert (diff > 0).mean() < 0.01, (name, levels)


def _scenes():
    from pano360_amd import synth
    for name in SCENES:
        g = load_golden(name)
        yield (name,) + tuple(scene_inputs(g))
    imgs, rots, intrs = synth.make_scene(4, 300, 170, sweep_deg=60.0, jitter=0.01, seed=68, kind="A")
    yield "noise 300 x 170", imgs, rots, intrs, 10 ** 9
    imgs, rots, intrs = synth.make_scene(3, 24, 14, sweep_deg=50.0, jitter=0.01, seed=3, kind="A")
    yield "tiny", imgs, rots, intrs, 10 ** 9


def test_oracle_float_mosaic_within_the_bound(oracle):
    """Criterion 2 of the GPU tests on the CPU: the float32 oracle's float mosaic is within E of
    the float64 truth at every pixel, for L = 1, 2, 5, 6 and 8 - so E was not tuned to the GPU."""
    rows = []
    for name, imgs, rots, intrs, mr in _scenes():
        for levels in (1, 2, 5, 6, 8):
            plan, patches, _ = oracle.warp_all(imgs, rots, intrs, True, mr)
            truth, s, overlap = mf.multiband_f64(patches, plan.shape, levels)
            _, ref_f = oracle.multiband_blend(patches, plan.shape, levels, return_float=True)
            e = mf.normalised_error(ref_f, truth, s)
            E = mf.bound(mf.max_taps(levels), levels, overlap)
            rows.append(f"{name} L={levels}: {e.max():.3f} (E {E:.0f})")
            assert e.max() <= E, (name, levels, float(e.max()), E)
            if levels == 1:
                assert e.max() == 0.0        # no blur: sharp weights, one exact product per pixel
    print("oracle worst e: " + "; ".join(rows))
