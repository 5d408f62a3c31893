"""CPU: the restatement of the reference's seam finder (tests/graph_cut_model.py) - its class
sweep against its literal heap loop, both against what the reference produced
(tests/golden/graph_cut_*.npz, tools/gen_graph_cut_golden.py) - the new exports' place in the C
ABI, the input domain of ``blend.graph_cut`` and the top-level ``blend`` shim."""
import glob
import inspect
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import graph_cut_model as gm

CASES = ("smooth", "alpha", "noise", "islands", "odd", "shrink14", "uint8")
EXPORTS = ("pano_seam_levels", "pano_seam_flood", "pano_seam_mask", "pano_alpha_blend")


def load(name):
    g = dict(np.load(os.path.join(GOLDEN, f"graph_cut_{name}.npz")))
    dtype = np.dtype(str(g["dtype"]))
    return g["img1"].astype(dtype), g["img2"].astype(dtype), int(g["shrink"]), g


def test_fixtures_are_the_listed_cases():
    found = sorted(os.path.basename(p)[10:-4]
                   for p in glob.glob(os.path.join(GOLDEN, "graph_cut_*.npz")))
    assert found == sorted(CASES)
    kinds = {name: load(name) for name in CASES}
    assert kinds["alpha"][0].shape[2] == 4 and kinds["alpha"][0].dtype == np.float32
    assert (kinds["alpha"][0][..., 3] == 0).any() and (kinds["alpha"][1][..., 3] == 0).any()
    assert kinds["uint8"][0].dtype == np.uint8 and kinds["shrink14"][2] == 14
    assert kinds["noise"][2] == 1 and kinds["smooth"][2] == 5
    h, w = kinds["odd"][0].shape[:2]
    assert h % kinds["odd"][2] and w % kinds["odd"][2]


@pytest.mark.parametrize("name", CASES)
def test_sweep_and_heap_equal_the_references_labels(name):
    img1, img2, shrink, g = load(name)
    level = gm.levels(img1, img2, shrink)
    border = gm.border_of(shrink)
    assert level.shape == g["labels"].shape
    if border == 1:
        assert (g["labels"] == 1).all() and not g["mask"].any()
        lab, mask = gm.graph_cut(img1, img2, shrink)
        assert np.array_equal(lab, g["labels"]) and np.array_equal(mask, g["mask"])
        return
    sweep, worked = gm.flood_sweep(level, border, want_stats=True)
    assert np.array_equal(sweep, g["labels"])
    assert np.array_equal(gm.flood_heap(level, border), g["labels"])
    # a seam worth the name: both labels hold a tenth of the grid, twenty classes did work
    assert min(np.mean(sweep == -1), np.mean(sweep == 1)) >= 0.10 and worked >= 20
    assert not (sweep == 0).any()


@pytest.mark.parametrize("name", CASES)
def test_mask_from_labels_equals_the_references_bytes(name):
    img1, img2, shrink, g = load(name)
    mask = gm.mask_from_labels(g["labels"], *img1.shape[:2])
    assert mask.dtype == np.uint8 and mask.shape == g["mask"].shape
    assert np.array_equal(mask, g["mask"])
    assert np.array_equal(gm.graph_cut(img1, img2, shrink)[1], g["mask"])


def test_islands_are_taken_late():
    """The island scene holds pockets of a high level that the flood cannot reach while it works
    through the levels above their walls': a "highest level first, nearest seed" shortcut gets
    them wrong."""
    img1, img2, shrink, g = load("islands")
    level = gm.levels(img1, img2, shrink)
    part_way = gm.flood_sweep(level, gm.border_of(shrink), stop_below=20)
    waiting = (part_way == 0) & (level >= 150)
    assert int(waiting.sum()) >= 100, int(waiting.sum())
    # ... and both colours take some of them in the end
    assert {-1, 1} <= set(g["labels"][waiting].tolist())


def random_level_grid(rng):
    rows, cols = int(rng.integers(1, 40)), int(rng.integers(5, 70))
    shrink = int(rng.choice([1, 2, 3, 5, 7, 13]))
    border = gm.border_of(shrink)
    cols = max(cols, 2 * border + 1 + int(rng.integers(0, 4)))
    span = int(rng.choice([2, 4, 16, 256]))
    level = rng.integers(0, span, (rows, cols)).astype(np.int16)
    if rng.random() < 0.5:                          # smooth it: long runs and big components
        level = np.maximum.accumulate(level, axis=int(rng.integers(0, 2))) // 2
    if rng.random() < 0.6:                          # alpha holes
        holes = rng.random((rows, cols)) < rng.uniform(0.02, 0.4)
        level[holes] = -1
    return level, border


def test_sweep_equals_heap_on_random_grids():
    rng = np.random.default_rng(20260)
    seen_low = 0
    for _ in range(120):
        level, border = random_level_grid(rng)
        sweep = gm.flood_sweep(level, border)
        assert np.array_equal(sweep, gm.flood_heap(level, border)), (level.shape, border)
        assert not (sweep == 0).any()
        seen_low += int((level < 0).any())
    assert seen_low >= 30


def test_uint8_levels_follow_the_wrapped_key():
    a = np.array([[[3], [5], [7], [0]]], np.uint8)
    b = np.array([[[5], [3], [7], [255]]], np.uint8)
    # differences 254, 2, 0, 1 -> priorities 253, 1, 255, 0
    assert gm.levels(a, b, 1).tolist() == [[253, 1, 255, 0]]
    assert gm.levels(a.astype(np.int16), b.astype(np.int16), 1).tolist() == [[2, 2, 0, 255]]


def test_small_grids_and_presets():
    with pytest.raises(ValueError):
        gm.presets(0, 20, 3)
    with pytest.raises(ValueError):
        gm.presets(4, 6, 3)
    lab = gm.presets(2, 7, 3)
    assert lab.tolist() == [[-1, -1, -1, -1, 1, 1, 1]] * 2
    assert (gm.presets(3, 9, 1) == 1).all()


def test_alpha_blend_model_is_numpys_expression():
    rng = np.random.default_rng(8)
    for dtype in (np.uint8, np.int16, np.int32, np.float32, np.float64):
        a = rng.integers(0, 256, (9, 14, 3)).astype(dtype)
        b = rng.integers(0, 256, (9, 14, 3)).astype(dtype)
        ramp = np.linspace(1, 0, 14).reshape((1, 14, 1))
        assert np.array_equal(gm.alpha_blend(a, b), (a * ramp + b * (1 - ramp)).astype("uint8"))
        for mdtype in (np.float32, np.float64):
            for shape in ((9, 14, 1), (9, 14, 3), (1, 14, 1)):
                mask = rng.random(shape).astype(mdtype)
                want = a * mask + b * (1 - mask)
                assert want.dtype == np.result_type(dtype, mdtype)
                assert np.array_equal(gm.alpha_blend(a, b, mask), want.astype("uint8"))


def test_seam_exports_are_declared_and_bound():
    from pano360_amd import _lib
    assert set(EXPORTS) <= set(_lib.EXPORTS)
    assert _lib.SEAM_DTYPES == {"uint8": 0, "int16": 1, "int32": 2, "float32": 3, "float64": 4}
    cells = _lib.SEAM_RESIDENT_CELLS
    assert 2 * cells + 512 <= 160 * 1024
    assert (216 + 2) * (195 + 2) <= cells           # the reference main()'s grid is resident
    src = open(os.path.join(ROOT, "pano360_amd", "csrc", "Makefile")).read()
    assert "graphcut.hip" in src and "-ffp-contract=off" in src


def test_float_taps_are_the_models():
    from pano360_amd import blend
    for n_out, n_in in ((976, 195), (1080, 216), (157, 52), (203, 67), (90, 6), (60, 4), (5, 5)):
        tab = blend._float_taps(n_out, n_in)
        taps, weights = gm.resize_taps(n_out, n_in)
        assert np.array_equal(tab[:, :2], taps)
        assert np.array_equal(tab[:, 2:].view(np.float32), weights)
        assert tab[:, :2].min() >= 0 and tab[:, :2].max() <= n_in - 1


def test_input_domain_errors_come_before_the_library(monkeypatch):
    from pano360_amd import _lib, blend, engine

    def no_engine():
        raise AssertionError("the device was touched")

    monkeypatch.setattr(engine, "engine", no_engine)
    monkeypatch.setattr(_lib, "lib", no_engine)
    ok = np.zeros((40, 60, 3), np.int16)
    with pytest.raises(ValueError):
        blend.graph_cut(ok, np.zeros((40, 61, 3), np.int16))
    with pytest.raises(ValueError):
        blend.graph_cut(np.zeros((40, 60, 5), np.int16), np.zeros((40, 60, 5), np.int16))
    with pytest.raises(ValueError):
        blend.graph_cut(ok, ok, shrink=0)
    with pytest.raises(ValueError):
        blend.graph_cut(ok, ok, shrink=2.5)
    with pytest.raises(ValueError):                 # 60 // 5 = 12 columns >= 7, 30 // 5 = 6 < 7
        blend.graph_cut(np.zeros((40, 30, 3), np.int16), np.zeros((40, 30, 3), np.int16))
    with pytest.raises(ValueError):                 # no rows
        blend.graph_cut(np.zeros((3, 60, 3), np.int16), np.zeros((3, 60, 3), np.int16))
    with pytest.raises(NotImplementedError):
        blend.graph_cut(ok.astype(np.int64), ok.astype(np.int64))
    with pytest.raises(NotImplementedError):
        blend.graph_cut(ok, ok.astype(np.int32))
    for value in (0.5, 256, -1, np.nan):
        bad = ok.astype(np.float64)
        bad[3, 4, 1] = value
        with pytest.raises(NotImplementedError):
            blend.graph_cut(bad, ok.astype(np.float64))
    with pytest.raises(NotImplementedError):
        blend.graph_cut(ok + 300, ok)
    with pytest.raises(OverflowError):              # what the reference raises under NumPy 2
        blend.graph_cut(np.zeros((40, 60, 4), np.uint8), np.zeros((40, 60, 4), np.uint8))
    with pytest.raises(ValueError):
        blend.alpha_blend(ok, ok[:, :10])
    with pytest.raises(NotImplementedError):
        blend.alpha_blend(ok, ok, np.ones((40, 60, 1), np.int32))


def test_top_level_blend_resolves_the_seam_calls():
    import blend
    from pano360_amd import blend as product
    assert blend.graph_cut is product.graph_cut and blend.alpha_blend is product.alpha_blend
    assert list(inspect.signature(blend.graph_cut).parameters) == ["img1", "img2", "shrink"]
    assert inspect.signature(blend.graph_cut).parameters["shrink"].default == 5
    assert list(inspect.signature(blend.alpha_blend).parameters) == ["img1", "img2", "mask"]
    assert list(inspect.signature(product.graph_cut_device).parameters)[:5] == [
        "img1", "img2", "shrink", "eng", "want_labels"]
    assert list(inspect.signature(product.blend_overlap_device).parameters)[:5] == [
        "img1", "img2", "delta", "blender", "shrink"]
    assert "astype(np.int16)" in product.graph_cut.__doc__
    assert not hasattr(blend, "warp") and "warp" in blend.__doc__
