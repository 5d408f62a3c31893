"""CPU: the float64 restatement of the Poisson blend's two operators (tests/poisson_model.py)
against what the reference produced (tests/golden/poisson_*.npz, tools/gen_poisson_golden.py),
the new export's place in the C ABI, and the top-level ``blend`` shim."""
import inspect
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import poisson_model as pm

CASES = ("ellipse128", "corners", "ellipse260")
GUARD = 1e-4


def load(name):
    return np.load(os.path.join(GOLDEN, f"poisson_{name}.npz"))


def test_fixture_masks_cover_the_special_places():
    """Between them the masks touch both last columns, column 0, the first and last rows, flat
    pixels 0 and N-1, and hold a hole and two components."""
    from scipy import ndimage
    seen = dict.fromkeys(("w-1", "w-2", "w-2 alone", "x0", "y0", "y-1", "first", "last", "hole",
                          "two"), False)
    for name in CASES:
        m = load(name)["mask"] != 0
        seen["w-1"] |= m[:, -1].any()
        seen["w-2"] |= m[:, -2].any()
        seen["w-2 alone"] |= (m[:, -2] & ~m[:, -1]).any()
        seen["x0"] |= m[:, 0].any()
        seen["y0"] |= m[0].any()
        seen["y-1"] |= m[-1].any()
        seen["first"] |= m[0, 0]
        seen["last"] |= m[-1, -1]
        seen["two"] |= ndimage.label(m)[1] >= 2
        # a hole: a background component that does not reach the border
        lab, n = ndimage.label(~m)
        border = set(lab[0]) | set(lab[-1]) | set(lab[:, 0]) | set(lab[:, -1])
        seen["hole"] |= any(k not in border for k in range(1, n + 1))
    assert all(seen.values()), seen


@pytest.mark.parametrize("name", CASES)
def test_model_operators_equal_the_references_products(name):
    g = load(name)
    mask = g["mask"]
    H, W = mask.shape
    for v, p_v, a_v in zip(g["vectors"], g["p_v"], g["a_v"]):
        v = v.astype(np.float64)
        # small integers: exact in any summation order
        assert np.array_equal(pm.apply_P(v, H, W), p_v.astype(np.float64))
        assert np.array_equal(pm.apply_A(v, mask), a_v.astype(np.float64))
        assert np.array_equal(pm.matrix_A(mask) @ v, a_v.astype(np.float64))


@pytest.mark.parametrize("name", CASES)
def test_model_solved_on_the_cpu_reproduces_the_reference(name):
    g = load(name)
    mask = g["mask"]
    inside = mask != 0
    sols, image = pm.solve(g["src"], g["tgt"], mask)
    for c in range(sols.shape[0]):
        assert np.abs(sols[c][inside] - g["sol"][c]).max() <= 1e-9
        # outside the mask the solution is the target
        assert np.array_equal(sols[c][~inside], g["tgt"][..., c][~inside].astype(np.float64))
    assert np.array_equal(image, g["result"])
    assert np.array_equal(g["result"][~inside], g["tgt"][~inside])


@pytest.mark.parametrize("name", CASES)
def test_fixture_leaves_few_pixels_in_the_guard_band(name):
    """The byte comparison of the GPU test leaves out the pixels whose solution is within the
    guard band of an integer; a fixture must keep them under 0.2 % of the mask per channel."""
    g = load(name)
    for sol in g["sol"]:
        assert np.mean(~pm.safe_pixels(sol, GUARD)) <= 0.002


def test_safe_pixels():
    sol = np.array([10.5, 11.00005, 10.99995, -3.0, -0.00005, 0.00005, 255.00005, 254.99995,
                    300.0, 300.00001, 12.0002])
    want = np.array([True, False, False, True, False, False, False, False, True, True, True])
    assert np.array_equal(pm.safe_pixels(sol, GUARD), want)


def test_poisson_export_is_declared_and_bound():
    from pano360_amd import _lib
    assert "pano_poisson_blend" in _lib.EXPORTS and _lib.ESOLVE == -4
    src = open(os.path.join(ROOT, "pano360_amd", "csrc", "Makefile")).read()
    assert "poisson.hip" in src


def test_top_level_blend_resolves_poisson_blend():
    import blend
    from pano360_amd import blend as product
    assert blend.poisson_blend is product.poisson_blend
    assert list(inspect.signature(blend.poisson_blend).parameters) == [
        "img_source", "img_target", "img_mask"]
    assert "SciPy" in product.poisson_blend.__doc__ and "poisson_matrix" in blend.__doc__
    assert not hasattr(blend, "poisson_matrix")
    params = inspect.signature(product.poisson_blend_device).parameters
    assert list(params)[:5] == ["src", "tgt", "mask", "eng", "want_solution"]
    assert "max_iters" in params
