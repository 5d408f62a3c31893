"""CPU: the view stage's host side (pano360_amd/view.py, the stitcher's --view / --equirect /
--cube flags) and its float64 model (tests/view_model.py) against brute force and identities."""
import math
import os
import re

import numpy as np
import pytest

import view_cases
import view_model as vm
from conftest import ROOT
from pano360_amd import _lib, view


# ------------------------------------------------------------------ mip chain
def test_model_mips_equal_the_brute_force_box_mean():
    img = view_cases.noise((33, 67), 11)
    levels = vm.mip_levels(img)
    assert [lv.shape[:2] for lv in levels] == [(33, 67), (17, 34), (9, 17), (5, 9), (3, 5), (2, 3),
                                               (1, 2), (1, 1)] == view.mip_shapes(33, 67)
    for src, dst in zip(levels, levels[1:]):
        h, w = src.shape[:2]
        for y in range(dst.shape[0]):
            for x in range(dst.shape[1]):
                for k in range(3):
                    block = [int(src[min(2 * y + j, h - 1), min(2 * x + i, w - 1), k])
                             for j in (0, 1) for i in (0, 1)]
                    assert dst[y, x, k] == (sum(block) + 2) >> 2
    assert [lv.shape[:2] for lv in vm.mip_levels(img[:1, :2])] == [(1, 2), (1, 1)]
    assert len(vm.mip_levels(img[:1, :1])) == 1


def test_mip_offsets_hold_every_level():
    for h, w in ((33, 67), (1, 2), (1, 1), (1400, 700), (32768, 32768)):
        shapes, offs = view.mip_shapes(h, w), view.mip_offsets(h, w)
        assert len(offs) == len(shapes) + 1 <= view.MAX_LEVELS + 1 and shapes[-1] == (1, 1)
        for (a, b), lo, hi in zip(shapes, offs, offs[1:]):
            assert lo % 256 == 0 and hi >= lo + 3 * a * b


# ------------------------------------------------------------------- geometry
def test_geometry_closed_open_and_cropped():
    g = view_cases.GEOMETRIES
    assert g["ring"].closed and g["sphere"].closed and g["tall"].closed and not g["open"].closed
    res = 2 * math.pi / 67
    assert view.MosaicGeometry((0, 0), (res, res), (10, 67)).closed
    assert not view.MosaicGeometry((0, 0), (res, res), (10, 66)).closed
    assert not view.MosaicGeometry((0, 0), (2 * math.pi / 67.6, res), (10, 67)).closed
    with pytest.raises(ValueError):
        view.MosaicGeometry((0, 0), (res, res), (10, 68))           # more than one turn
    crop = g["ring"].cropped((3, 5, 20, 40))
    assert crop.shape == (20, 40) and crop.resolution == g["ring"].resolution
    assert crop.low == (g["ring"].low[0] + 5 * g["ring"].resolution[0],
                        g["ring"].low[1] + 3 * g["ring"].resolution[1])
    assert not crop.closed and not g["ring"].cropped((0, 0, 33, 67)).closed     # never closed
    for bad in ((0, 0, 34, 67), (-1, 0, 3, 3), (0, 60, 3, 8), (0, 0, 0, 5)):
        with pytest.raises(ValueError):
            g["ring"].cropped(bad)


def test_geometry_of_a_plan():
    from pano360_amd import engine, synth
    rots, intrs = synth.make_cameras(5, 240, 136, sweep_deg=90.0)
    plan = engine.Plan([(136, 240)] * 5, rots, intrs, True, 1400)
    geom = view.MosaicGeometry.of_plan(plan)
    assert geom.shape == plan.shape and geom.low == tuple(plan.low)
    assert geom.resolution == tuple(plan.resolution) and not geom.closed


def test_cube_faces_are_rotations_that_look_along_their_axes():
    axes = ((0, 0, 1), (1, 0, 0), (0, 0, -1), (-1, 0, 0), (0, -1, 0), (0, 1, 0))
    faces = view.cube_faces(32)
    assert len(faces) == 6 == len(view.CUBE_FACES)
    for k, (face, axis) in enumerate(zip(faces, axes)):
        rot = view.face_rotation(k)
        assert np.array_equal(rot, view.face_rotation(view.CUBE_FACES[k]))
        assert np.allclose(rot.T @ rot, np.eye(3), atol=0) and np.linalg.det(rot) == pytest.approx(1)
        assert (face.kind, face.w, face.h) == (view.RECTILINEAR, 32, 32)
        centre = vm.directions(face, 15.5, 15.5)
        assert np.allclose(centre / np.linalg.norm(centre), axis, atol=1e-15)
        # f = side / 2: the edge of the first pixel is 45 degrees off the axis
        edge = vm.directions(face, -0.5, 15.5)
        assert edge @ np.array(axis, float) / np.linalg.norm(edge) == pytest.approx(math.sqrt(0.5))
    assert np.allclose(view.rotation(0.3, 0, 0) @ [0, 0, 1], [math.sin(0.3), 0, math.cos(0.3)])
    assert np.allclose(view.rotation(0, 0.3, 0) @ [0, 0, 1], [0, -math.sin(0.3), math.cos(0.3)])
    full = view.equirect(64)
    assert (full.w, full.h) == (64, 32)
    assert full.params == (-math.pi + math.pi / 64, math.pi / 32, -math.pi / 2 + math.pi / 64,
                           math.pi / 32)


# --------------------------------------------------------- identities (model)
@pytest.mark.parametrize("name", ["tall", "open", "sphere"])
def test_model_own_view_returns_the_mosaic(name):
    geom, img = view_cases.GEOMETRIES[name], view_cases.mosaic(name)
    got, mask = vm.render(vm.mip_levels(img), geom, geom.own_view())
    # the first and last rows (and, open, columns) sit ON the coverage boundary: rounding
    # decides whether they are covered; a covered pixel is the mosaic's either way
    keep = ~vm.near_boundary(geom.own_view(), geom)
    assert keep[1:-1, 1:-1].all() and mask[keep].all()
    if name == "sphere":
        # the forward step from the last row goes over the pole, where theta turns by pi: rho is
        # half the mosaic's width there and the row comes from the coarsest level
        assert vm.coordinates(geom.own_view(), geom)[3][-1].min() > 6
        got, img, mask, keep = got[:-1], img[:-1], mask[:-1], keep[:-1]
    assert np.array_equal(got[keep], img[keep])
    assert np.array_equal(got[mask == 1], img[mask == 1]) and not got[mask == 0].any()


@pytest.mark.parametrize("name, shift", [("tall", 7), ("tall", -50), ("sphere", 100)])
def test_model_shifted_own_view_rolls_a_closed_mosaic(name, shift):
    geom, img = view_cases.GEOMETRIES[name], view_cases.mosaic(name)
    got, mask = vm.render(vm.mip_levels(img), geom, geom.own_view(shift))
    want = np.roll(img, -shift, axis=1)
    if name == "sphere":                            # (its last row: see the test above)
        got, want, mask = got[:-1], want[:-1], mask[:-1]
    assert mask[1:].all() and np.array_equal(got[mask == 1], want[mask == 1])


# ------------------------------------------------------------- argument checks
def test_arguments_are_checked_before_the_device():
    good = np.zeros((4, 5, 3), np.uint8)
    geom = view.MosaicGeometry((0, 0), (0.1, 0.1), (4, 5))
    for bad in (good.astype(np.float32), good.astype(np.int16), good[..., :2], good[..., 0],
                np.zeros((4, 5, 4), np.uint8), np.zeros((0, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            view.mip_device(bad)
        with pytest.raises(ValueError):
            view.render_device(bad, geom, [view.equirect(8)])
    for size in (0, -3, (4, 0), 2.5):
        with pytest.raises(ValueError):
            view.perspective(0, 0, 0, 1.0, size)
        with pytest.raises(ValueError):
            view.cube_faces(size)
        with pytest.raises(ValueError):
            view.little_planet(size)
    for fov in (0.0, -1.0, math.pi, 4.0, float("nan")):
        with pytest.raises(ValueError):
            view.perspective(0, 0, 0, fov, (8, 8))
    for fov in (0.0, 2 * math.pi, float("nan")):
        with pytest.raises(ValueError):
            view.little_planet(8, fov)
    for width in (0, 1, 7):
        with pytest.raises(ValueError):
            view.equirect(width)
    with pytest.raises(ValueError):                 # the geometry is another mosaic's
        view.render_device(good, view.MosaicGeometry((0, 0), (0.1, 0.1), (5, 4)), [view.equirect(8)])
    with pytest.raises(ValueError):
        view.render_device(good, geom, [])
    with pytest.raises(ValueError):
        view.render_device(good, geom, [view.equirect(8)] * (view.MAX_VIEWS + 1))
    with pytest.raises(ValueError):
        view.render_device(good, geom, ["front"])


def test_view_records_fill_the_abi_structures():
    geom = view_cases.GEOMETRIES["ring"]
    views = view.cube_faces(8) + [view.equirect(16), view.little_planet(9, 3.0)]
    table, record = view.view_records(views, geom, geom.shape)
    assert len(table) == 8 and (record.h, record.w, record.closed) == (33, 67, 1)
    assert tuple(record.low) == geom.low and tuple(record.res) == geom.resolution
    for rec, v in zip(table, views):
        assert (rec.kind, rec.w, rec.h) == (v.kind, v.w, v.h)
        assert np.array_equal(np.array(rec.m[:]).reshape(3, 3), v.mat) and tuple(rec.p) == v.params
    # the module's names are the binding's constants, and the model's
    assert (view.MAX_LEVELS, view.MAX_VIEWS, view.MAX_SIDE) == (
        _lib.VIEW_MAX_LEVELS, _lib.VIEW_MAX_VIEWS, _lib.VIEW_MAX_SIDE)
    assert (view.RECTILINEAR, view.EQUIRECT, view.STEREOGRAPHIC) == (
        _lib.VIEW_RECTILINEAR, _lib.VIEW_EQUIRECT, _lib.VIEW_STEREOGRAPHIC)
    header = open(os.path.join(ROOT, "include", "pano360.h")).read()
    assert vm.MAX_LEVELS == view.MAX_LEVELS
    assert (vm.RECTILINEAR, vm.EQUIRECT, vm.STEREOGRAPHIC) == (view.RECTILINEAR, view.EQUIRECT, view.STEREOGRAPHIC)
    for name in ("pano_mip_u8", "pano_view_render"):
        assert name in _lib.EXPORTS and re.search(rf"\nint {name}\(pano_ctx \*ctx,", header)


# ----------------------------------------------------------------- command line
def test_stitcher_flags_parse_and_need_an_output():
    from pano360_amd import stitcher
    args = stitcher.parse_args(["dir"])
    assert args.view == [] and args.equirect is None and args.cube is None
    args = stitcher.parse_args(["dir", "--register", "-o", "out/pano.jpg", "--equirect", "4096", "--cube",
                                "1024", "--view", "0,0,90", "--view=-30.5,10,60,640x480"])
    assert args.view == [(0.0, 0.0, 90.0, (1920, 1080)), (-30.5, 10.0, 60.0, (640, 480))]
    assert (args.equirect, args.cube) == (4096, 1024)
    outputs = stitcher.view_outputs(args)
    assert [name for name, _ in outputs] == (
        ["out/pano_view0.jpg", "out/pano_view1.jpg", "out/pano_equirect.jpg"]
        + [f"out/pano_cube_{face}.jpg" for face in ("front", "right", "back", "left", "up", "down")])
    first, second = outputs[0][1], outputs[1][1]
    assert (first.w, first.h, second.w, second.h) == (1920, 1080, 640, 480)
    assert np.allclose(first.mat, view.perspective(0, 0, 0, math.pi / 2, (1920, 1080)).mat)
    assert np.allclose(second.mat, view.perspective(math.radians(-30.5), math.radians(10), 0,
                                                    math.radians(60), (640, 480)).mat)
    assert (outputs[2][1].w, outputs[2][1].h, outputs[3][1].w) == (4096, 2048, 1024)
    for flags in (["--view", "0,0,90"], ["--equirect", "64"], ["--cube", "8"],                # no -o
                  ["-o", "a.png", "--view", "0,0"], ["-o", "a.png", "--view", "0,0,180"],
                  ["-o", "a.png", "--view", "0,0,90,640"], ["-o", "a.png", "--view", "0,0,90,0x4"],
                  ["-o", "a.png", "--equirect", "63"], ["-o", "a.png", "--cube", "0"]):
        with pytest.raises(SystemExit):
            stitcher.parse_args(["dir"] + flags)


# ------------------------------------------ what the GPU comparisons leave out
@pytest.mark.parametrize("name", sorted(view_cases.CASES))
def test_gpu_cases_leave_out_at_most_one_percent(name):
    geom_name, views = view_cases.CASES[name]
    geom = view_cases.GEOMETRIES[geom_name]
    near = np.concatenate([vm.near_boundary(v, geom).ravel() for v in views])
    assert near.mean() <= 0.01, (name, int(near.sum()), near.size)
    for v in views:                                 # ... of every view with a hundred pixels or more
        share = vm.near_boundary(v, geom).mean()
        assert share <= 0.01 or v.w * v.h < 100, (name, share)


def test_the_levels_case_crosses_three_levels():
    geom = view_cases.GEOMETRIES["sphere"]
    n = len(view.mip_shapes(*geom.shape))
    assert len(vm.levels_crossed(view_cases.LEVELS_VIEW, geom, n)) >= 3
    # magnification: every pixel of the narrow views samples level 0 alone
    for name in ("ring_yaw3.0_fov0.3", "ring_yaw-3.1_fov0.3"):
        (v,), ring = view_cases.CASES[name][1], view_cases.GEOMETRIES["ring"]
        assert vm.levels_crossed(v, ring, 8) == {0}
        assert np.nanmax(vm.coordinates(v, ring)[3]) < 0
