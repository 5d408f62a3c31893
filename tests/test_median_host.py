"""CPU: the median blend's contract as ``median_model`` restates it, on
the oracle's patches: what it must equal where nothing moved, what it does to something that
moved through a dense sweep, and where it stops working."""
import re

import numpy as np
import pytest

import median_model
from conftest import ROOT, SCENES, load_golden, scene_inputs
from median_cases import bl_patches, ghost_region, ghost_rig


@pytest.mark.parametrize("name", SCENES)
def test_everything_agrees_is_the_linear_blend(oracle, name):
    """tol = 2 exceeds any difference of colours in [0, 1]: every sample is an inlier."""
    g = load_golden(name)
    imgs, rots, intrs, mr = scene_inputs(g)
    plan, patches, _ = oracle.warp_all(imgs, rots, intrs, False, mr)
    mosaic, valid = median_model.median_blend(patches, plan.shape, 2)
    assert np.array_equal(mosaic, oracle.linear_blend(patches, plan.shape))
    assert np.array_equal(mosaic, g["linear_mosaic"])
    assert np.array_equal(valid, g["lin_valid"])
    # ... and the vote does something on these scenes of unrelated noise frames
    voted, _ = median_model.median_blend(patches, plan.shape, 0.1)
    assert (voted != mosaic).any(axis=-1).mean() > 0.5


def test_stage_patches_agree_with_the_golden_linear_blend():
    g = load_golden("pure")
    shape = tuple(int(v) for v in g["bl_shape"])
    mosaic, valid = median_model.median_blend(bl_patches(g), shape, 2)
    assert np.array_equal(mosaic, g["bl_linear"])
    assert np.array_equal(valid, g["bl_valid"])


def test_two_samples_the_heavier_one_is_the_median():
    """The ownership rule: with two samples j is the one of larger weight, the earlier on a tie."""
    def patch(colour, alpha):
        w = np.zeros((1, 3, 4), np.float32)
        w[..., :3], w[..., 3] = colour, alpha
        return w, np.zeros((1, 3), bool), np.s_[0:1, 0:3]
    patches = [patch(0.9, [0.2, 0.1, 0.2]), patch(0.1, [0.1, 0.2, 0.2])]
    present, colour, alpha = median_model.stack(patches, (1, 3))
    j, total = median_model.median_index(present, colour, alpha)
    # (on the tie the lower KEY comes first in the sorted order and reaches half the weight)
    assert j.tolist() == [[0, 1, 1]] and (total > 0).all()
    mosaic, _ = median_model.median_blend(patches, (1, 3), 0.1)
    assert mosaic[0, :, 0].tolist() == [int(np.float32(255) * np.float32(0.9)),
                                        int(np.float32(255) * np.float32(0.1)),
                                        int(np.float32(255) * np.float32(0.1))]


def test_ghost_is_voted_out_of_a_dense_sweep(oracle):
    shape, clean, painted, _ = ghost_rig(oracle, 8)
    assert shape == (55, 132)
    region = ghost_region(shape, clean, painted)
    assert region.sum() == 324
    present, colour, alpha = median_model.stack(painted, shape)
    assert present.sum(axis=0)[region].min() >= 7
    w = median_model.weights(present, alpha)
    share = w[4] / np.maximum(w.sum(axis=0), 1)
    assert 0.25 < share[region].max() < 0.26          # (0.254: far from half the weight)

    med_clean, _ = median_model.median_blend(clean, shape, 0.1)
    med_painted, _ = median_model.median_blend(painted, shape, 0.1)
    lin_clean = oracle.linear_blend(clean, shape)
    lin_painted = oracle.linear_blend(painted, shape)
    assert np.array_equal(med_clean, lin_clean)
    dev = np.abs(med_painted.astype(int) - med_clean.astype(int))
    assert dev[~region].max() == 0
    # the painted sample is dropped: one consistent sample less in a weighted mean moves it by at
    # most the spread d of the clean samples (+ 1 level for the two quantisations)
    pc, cc, _ = median_model.stack(clean, shape)
    hi = np.where(pc[..., None], cc, -np.inf).max(axis=0)
    lo = np.where(pc[..., None], cc, np.inf).min(axis=0)
    d = (hi - lo).max(axis=-1)
    assert (dev[region] <= (255 * d[region] + 1)[:, None]).all()
    print("median deviation in the ghost region: max", dev[region].max())
    lin_dev = np.abs(lin_painted.astype(int) - lin_clean.astype(int)).max(axis=-1)[region]
    print("linear deviation in the ghost region: max", lin_dev.max(), "median", np.median(lin_dev))
    assert np.median(lin_dev) > 20


def test_weight_share_limit(oracle):
    """The vote is a weighted majority: at 20 degrees between frames the painted frame holds more
    than half the weight around its centre, IS the median there, and the object survives."""
    shape, clean, painted, _ = ghost_rig(oracle, 20)
    region = ghost_region(shape, clean, painted)
    present, colour, alpha = median_model.stack(painted, shape)
    w = median_model.weights(present, alpha)
    share = w[4] / np.maximum(w.sum(axis=0), 1)
    heavy = region & (share > 0.5)
    assert heavy.sum() > 100
    j, _ = median_model.median_index(present, colour, alpha)
    assert (j[heavy] == 4).all()
    med_clean, _ = median_model.median_blend(clean, shape, 0.1)
    med_painted, _ = median_model.median_blend(painted, shape, 0.1)
    dev = np.abs(med_painted.astype(int) - med_clean.astype(int)).max(axis=-1)
    assert np.median(dev[heavy]) > 100                 # magenta, not the scene
    assert dev[~region].max() == 0


def test_binding_declares_the_median_entry_points():
    from pano360_amd import _lib, stitcher
    header = open(f"{ROOT}/include/pano360.h").read()
    for name in ("pano_median_cameras", "pano_median_blend"):
        assert name in _lib.EXPORTS and re.search(rf"\nint {name}\(pano_ctx \*ctx,", header)
    assert stitcher.BLENDERS["median"] is stitcher.median_blend
    assert stitcher._FUSED[stitcher.median_blend] == "median" and stitcher.GHOST_TOL == 0.1


def test_command_line_tolerance():
    from pano360_amd import stitcher
    assert stitcher.parse_args(["dir", "-b", "median"]).ghost_tol is None
    assert stitcher.parse_args(["dir", "-b", "median", "--ghost-tol", "0.25"]).ghost_tol == 0.25
    assert stitcher.parse_args(["dir", "-b", "median", "--ghost-tol", "0"]).ghost_tol == 0
    for bad in (["dir", "--ghost-tol", "0.1"], ["dir", "-b", "linear", "--ghost-tol", "0.1"],
                ["dir", "-b", "median", "--ghost-tol", "-0.1"],
                ["dir", "-b", "median", "--ghost-tol", "nan"]):
        with pytest.raises(SystemExit):
            stitcher.parse_args(bad)
