"""CPU: the fill stage's float64 model (tests/fill_model.py) against the properties a pull-push
fill must have, the host side of pano360_amd/fill.py (levels, workspace, bindings), the stitcher's
--fill flag, and the condition on the inputs of tests/test_gpu_fill.py."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fill_cases
import fill_model as fm
from conftest import ROOT
from pano360_amd import _lib, fill, view


# ------------------------------------------------------------ model properties
def _example(closed=False):
    img = fill_cases.noise(37, 53, 5)
    mask = fm.blobs(37, 53, 9, 6.0, seed=3)
    return img, mask, fm.fill(img, mask, closed)


def test_model_keeps_valid_pixels_and_stays_within_their_range():
    img, mask, (out, f0) = _example()
    assert 0 < mask.sum() < mask.size
    assert np.array_equal(out[mask != 0], img[mask != 0])
    for k in range(3):
        lo, hi = img[..., k][mask != 0].min(), img[..., k][mask != 0].max()
        assert lo <= f0[..., k].min() and f0[..., k].max() <= hi
        assert lo <= out[..., k].min() and out[..., k].max() <= hi


def test_model_constant_image_stays_constant():
    mask = fm.blobs(21, 30, 5, 5.0, seed=1)
    img = np.empty((21, 30, 3), np.uint8)
    img[:] = (17, 130, 255)
    garbage = np.where(mask[..., None] != 0, img, 99).astype(np.uint8)      # holes hold anything
    for closed in (False, True):
        assert np.array_equal(fm.fill(garbage, mask, closed)[0], img)


def test_model_one_valid_pixel_paints_the_image():
    img = fill_cases.noise(19, 45, 2)
    mask = np.zeros((19, 45), np.uint8)
    mask[11, 30] = 1
    for closed in (False, True):
        out, _ = fm.fill(img, mask, closed)
        assert (out == img[11, 30]).all()


def test_model_all_valid_and_none_valid_return_the_input():
    img = fill_cases.noise(9, 14, 4)
    for mask in (np.ones((9, 14), np.uint8), np.zeros((9, 14), np.uint8)):
        out, _ = fm.fill(img, mask)
        assert np.array_equal(out, img)


def test_model_closed_acts_next_to_a_hole_over_column_0_only():
    h, w = 64, 96
    img = fill_cases.noise(h, w, 8)
    mask = np.ones((h, w), np.uint8)
    mask[20:29, :5] = 0                             # a hole across column 0: 5 columns left, 4 right
    mask[20:29, -4:] = 0
    mask[40:44, 50:55] = 0                          # ... and one far from it
    open_, closed = fm.fill(img, mask, False)[0], fm.fill(img, mask, True)[0]
    differs = (open_ != closed).any(axis=-1)
    assert differs[20:29, :5].any() and differs[20:29, -4:].any()
    # no further than the hole's reach: only its own pixels can change
    seam_hole = np.zeros((h, w), bool)
    seam_hole[20:29, :5] = seam_hole[20:29, -4:] = True
    assert not differs[~seam_hole].any()


# ------------------------------------------------------------ levels, workspace
def test_levels_and_workspace_layout():
    assert fill.TAIL_PIXELS == 4096 and fm.level_shapes(33, 67) == view.mip_shapes(33, 67)
    for h, w in ((1, 1), (1, 7), (64, 64), (65, 64), (1, 4096), (1, 4097), (2474, 13760),
                 (32768, 32768)):
        shapes, offs = fill.level_shapes(h, w), fill.level_offsets(h, w)
        assert shapes == fm.level_shapes(h, w) and shapes[-1] == (1, 1)
        assert len(offs) == len(shapes) + 1 and offs[0] == 0
        for (a, b), lo, hi in zip(shapes[1:], offs[1:], offs[2:]):
            assert lo % 256 == 0 and lo >= fill.HEADER and hi >= lo + fill.TEXEL * a * b
        tail = fill.tail_level(h, w)
        assert shapes[tail][0] * shapes[tail][1] <= 4096
        assert all(a * b > 4096 for a, b in shapes[:tail])
        # what the tail's workgroup holds in LDS: its level and everything below
        assert fill.TEXEL * sum(a * b for a, b in shapes[tail:]) <= 128 * 1024
    assert fill.tail_level(64, 64) == 0 and fill.launches(64, 64) == (0, 0)
    assert fill.tail_level(65, 64) == 1 and fill.launches(65, 64) == (0, 1)
    assert fill.launches(2474, 13760) == (6, 7)
    for bad in ((0, 5), (5, 0), (32769, 1)):
        with pytest.raises(ValueError):
            fill.level_shapes(*bad)


def test_native_layout_equals_the_python_one():
    """csrc/fill_layout.h is plain C++: a host program prints what pano_fill_u8 will use."""
    shapes = [(1, 1), (1, 7), (64, 64), (65, 64), (131, 257), (611, 1103), (1, 4097), (2474, 13760),
              (32768, 32768)]
    body = "".join(f"show({h}, {w});" for h, w in shapes)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "lay.cpp"), os.path.join(tmp, "lay")
        with open(src, "w") as fid:
            fid.write('#include <stdio.h>\n#include "fill_layout.h"\n'
                      'static void show(int h, int w) { FillLayout L; if (!fill_layout(h, w, &L)) return;'
                      'printf("%d %d %lld %d", L.n, L.tail, (long long)L.bytes, L.lds[L.n]);'
                      'for (int l = 0; l < L.n; ++l) printf(" %d %d %lld", L.h[l], L.w[l], (long long)L.off[l]);'
                      'printf("\\n"); }\n'
                      f'int main() {{ {body} FillLayout L; '
                      'printf("%d %d\\n", fill_layout(0, 4, &L), fill_layout(4, 32769, &L)); return 0; }\n')
        subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "pano360_amd", "csrc"),
                               src, "-o", exe])
        lines = subprocess.check_output([exe]).decode().splitlines()
    assert lines[-1] == "0 0" and len(lines) == len(shapes) + 1
    for (h, w), line in zip(shapes, lines):
        got = [int(v) for v in line.split()]
        levels, offs = fill.level_shapes(h, w), fill.level_offsets(h, w)
        tail = fill.tail_level(h, w)
        assert got[:4] == [len(levels), tail, offs[-1], sum(a * b for a, b in levels[tail:])]
        assert got[4:] == [v for (a, b), off in zip(levels, offs) for v in (a, b, off)]


def test_header_and_binding_agree():
    assert fill.TAIL_PIXELS == _lib.FILL_TAIL_PIXELS and view.MAX_SIDE == _lib.VIEW_MAX_SIDE
    assert {"pano_fill_u8", "pano_select_u8"} <= set(_lib.EXPORTS)


# ------------------------------------------------------------ argument checks
def test_arguments_are_checked_before_the_device():
    good, mask = np.zeros((4, 5, 3), np.uint8), np.ones((4, 5), np.uint8)
    for bad in (good.astype(np.float32), good[..., :2], good[..., 0], np.zeros((0, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            fill.fill_device(bad, mask)
    for bad in (mask[:3], mask.astype(np.float32), mask[..., None]):
        with pytest.raises(ValueError):
            fill.fill_device(good, bad)
    for width in (0, 1, 7):
        with pytest.raises(ValueError):
            fill.sphere_geometry(width)


def test_sphere_geometry_covers_every_direction():
    geom = fill.sphere_geometry(64)
    assert geom.shape == (34, 64) and geom.closed
    sa, sb = 2 * np.pi / 64, np.pi / 32
    assert geom.low == (-np.pi + sa / 2, -np.pi / 2 - sb / 2) and geom.resolution == (sa, sb)
    # the poles lie half a row inside the first and the last row
    for phi in (-np.pi / 2, np.pi / 2):
        fy = (phi - geom.low[1]) / geom.resolution[1]
        assert 0.49 < fy < geom.shape[0] - 1 - 0.49
    eq = view.equirect(64)                          # rows 1 .. 32 are the equirect's
    assert geom.low[1] + geom.resolution[1] == pytest.approx(eq.params[2], abs=1e-15)
    assert (geom.low[0], geom.resolution) == (eq.params[0], (eq.params[1], eq.params[3]))
    res = 2 * np.pi / 1000.4
    assert fill.sphere_width(view.MosaicGeometry((0, 0), (res, res), (10, 500))) == 1000
    assert fill.sphere_width(view.MosaicGeometry((0, 0), (1e-4, 1e-4), (10, 500))) == 4096
    assert fill.sphere_width(view.MosaicGeometry((0, 0), (5.0, 1.0), (1, 1))) == 2


# ----------------------------------------------------------------- command line
def test_stitcher_fill_flag_parses_and_refuses_crop():
    from pano360_amd import stitcher
    assert stitcher.parse_args(["dir"]).fill is False
    args = stitcher.parse_args(["dir", "--fill", "-o", "m.jpg", "--cube", "64"])
    assert args.fill and not args.crop
    for flags in (["--fill", "--crop"], ["--fill", "-c", "-o", "m.jpg"]):
        with pytest.raises(SystemExit):
            stitcher.parse_args(["dir"] + flags)


# ------------------------------------------ what the GPU comparisons leave out
@pytest.mark.parametrize("name", fill_cases.CASES)
def test_gpu_cases_have_few_near_ties(name):
    """A condition on the inputs, not on the kernel: at most 2 % of a case's hole values lie within
    the band in which float32 may round to the other side."""
    img, mask, closed, want, f0 = fill_cases.case(name)
    assert want.shape == img.shape and np.array_equal(want[mask != 0], img[mask != 0])
    holes = mask == 0
    if not holes.any() or not (mask != 0).any():
        assert np.array_equal(want, img)
        return
    near = fm.near_tie(f0)[holes]
    assert near.mean() <= 0.02, (name, int(near.sum()), near.size)
