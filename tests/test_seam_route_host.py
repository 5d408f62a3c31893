"""CPU: the seam routing's contract as ``seam_route_model`` restates it:
the literal heap loop against the class sweep on random and forged grids, the faults the forged
grids catch, the colouring, what the owner map promises the blur and the collapse, and the
command line."""
import re

import numpy as np
import pytest

import seam_route_cases as sc
import seam_route_model as sm
from conftest import ROOT


def random_planes(rng):
    """A Voronoi partition of 1 .. 40 x 3 .. 80 cells among 2 .. 7 cameras (a: the nearest site,
    second: the runner-up), open where the two distances are close or at random, with a palette of
    2 .. 256 levels, walls, and open islands for pairs of cameras dropped into the seeds."""
    rows, cols = int(rng.integers(1, 41)), int(rng.integers(3, 81))
    cams = int(rng.integers(2, 8))
    y, x = np.mgrid[:rows, :cols]
    sites = np.stack([rng.uniform(-2, rows + 2, cams), rng.uniform(-2, cols + 2, cams)], axis=1)
    dist = np.hypot(y[None] - sites[:, 0, None, None], x[None] - sites[:, 1, None, None])
    ranked = np.argsort(dist, axis=0, kind="stable")
    a, second = ranked[0], ranked[1]
    near = np.sort(dist, axis=0)
    opened = (near[1] - near[0] < rng.uniform(1, 12)) | (rng.random((rows, cols)) < rng.choice([0, 0.3]))
    palette = [np.array([0, 255]), np.array([0, 1, 255]), rng.integers(0, 256, 8),
               np.arange(256)][int(rng.integers(0, 4))]
    level = rng.choice(palette, (rows, cols))
    wall = rng.random((rows, cols)) < rng.choice([0, 0.05, 0.25])
    for _ in range(int(rng.integers(0, 3))):                # islands
        yy, xx = int(rng.integers(0, rows)), int(rng.integers(0, cols))
        box = np.s_[yy:yy + int(rng.integers(1, 5)), xx:xx + int(rng.integers(1, 5))]
        pair = rng.choice(cams, 2, replace=False)
        a[box], second[box], opened[box] = pair[0], pair[1], True
    return sc.planes_from(a, second, level, opened, wall, cams)


def test_heap_loop_equals_class_sweep_on_random_grids():
    rng = np.random.default_rng(2025)
    sizes, groups, unreached = set(), set(), 0
    for k in range(260):
        a, second, diff, label, group, n, n_groups = random_planes(rng)
        heap = sm.flood_heap(a, second, diff, label, group)
        sweep = sm.flood_sweep(a, second, diff, label, group)
        assert np.array_equal(heap, sweep), f"grid {k} {label.shape}, {n} cameras"
        # seeds and walls never change; an open pixel takes one of its two cameras or stays
        fixed = label != sm.OPEN
        assert np.array_equal(heap[fixed], label[fixed])
        took = heap[~fixed]
        assert ((took == a[~fixed]) | (took == second[~fixed]) | (took == sm.OPEN)).all()
        sizes.add(label.shape)
        groups.add(n_groups)
        unreached += int((took == sm.OPEN).any())
    print(f"{len(sizes)} sizes, group counts {sorted(groups)}, {unreached} grids with unreached pixels")
    assert len(sizes) > 200 and max(groups) >= 4 and unreached >= 20


@pytest.mark.parametrize("name", sc.PLANES)
def test_forged_planes_heap_equals_sweep(name):
    heap, owner, worked = sc.truth(name)                    # (asserts the equality itself)
    a, second, diff, label, group, n, n_groups = sc.PLANES[name]
    assert worked >= 1 and owner.min() >= -1 and owner.max() < n
    assert (label == sm.OPEN).any() and len(group) == n and group.max() == n_groups - 1


def test_forged_planes_reach_what_they_are_for():
    # pickets: walls on both sides of a 64-cell border of both axes
    label = sc.PLANES["valley-65x129"][3]
    assert (label[:, [63, 64, 127, 128]] == sm.WALL).any(axis=0).all() and (label[[63, 64]] == sm.WALL).any()
    # the serpentine's corridor is taken by camera 1 alone, in one class
    for name in sc.SERPENTINES:
        a, second, diff, label, group, _, _ = sc.PLANES[name]
        heap = sc.truth(name)[0]
        assert (heap[diff == 255] == 1).all() and (diff == 255).sum() > 6000
    # three groups meet
    assert sc.PLANES["three-at-a-point-67x90"][6] == 3
    owner = sc.truth("three-at-a-point-67x90")[1]
    assert {0, 1, 2} <= set(owner[30:37, 41:49].ravel().tolist())
    # cells that admit 0 directly above cells that admit 2, both unlabelled at the start
    a, second, diff, label, group, _, _ = sc.PLANES["same-group-neighbours-40x70"]
    assert ((label[19] == sm.OPEN) & (a[19] == 0) & (label[20] == sm.OPEN) & (a[20] == 2)).sum() > 30
    # labels beyond a byte
    owner = sc.truth("far-indices-20x70")[1]
    assert {0, 300, 32000} <= set(owner.ravel().tolist())
    moved = (owner != sc.PLANES["far-indices-20x70"][0]) & (owner >= 0)
    assert moved.any()
    # the island keeps a: nothing is labelled 3 or 4 and nothing of {0, 1} gets into the pocket
    heap, owner, _ = sc.truth("island-40x90")
    assert (heap[5:9, 3:8] == sm.OPEN).all() and (owner[5:9, 3:8] == 3).all()
    assert (heap[21:26, 3:8] == sm.OPEN).all() and (owner[21:26, 3:8] == 0).all()


@pytest.mark.parametrize("fault", ("connect8", "strict", "reverse_groups", "ignore_admissible"))
def test_each_fault_changes_labels_on_the_forged_planes(fault):
    """A device flood with 8-connectivity, ``D > d``, the groups in reverse or no admissibility
    cannot pass tests/test_gpu_seam_route.py: each changes labels on these grids."""
    caught = []
    for name, (a, second, diff, label, group, _, _) in sc.PLANES.items():
        wrong = sm.flood_sweep(a, second, diff, label, group, **{fault: True})
        if not np.array_equal(wrong, sc.truth(name)[0]):
            caught.append(name)
    print(f"{fault}: caught by {caught}")
    assert caught


def test_greedy_groups_are_a_proper_colouring():
    rng = np.random.default_rng(7)
    for _ in range(200):
        n = int(rng.integers(1, 12))
        pairs = (rng.random((n, n)) < rng.uniform(0, 0.6)).astype(np.uint8)
        np.fill_diagonal(pairs, 0)
        group, n_groups = sm.groups_of(pairs)
        compete = (pairs | pairs.T).astype(bool)
        for c in range(n):
            assert not (group[compete[c]] == group[c]).any()
            # greedy: every smaller colour is taken by a lower-indexed competitor
            assert set(range(group[c])) <= set(group[:c][compete[c, :c]].tolist())
        assert n_groups == group.max() + 1
    # a ring of six cameras: two groups; of five: three
    def ring(n):
        return np.roll(np.eye(n, dtype=np.uint8), 1, axis=1)
    assert sm.groups_of(ring(6))[0].tolist() == [0, 1, 0, 1, 0, 1]
    assert sm.groups_of(ring(5))[0].tolist() == [0, 1, 0, 1, 2]


@pytest.mark.parametrize("name", sc.PATCHES)
def test_every_owner_has_alpha_at_its_pixel(name):
    patches, shape, ratio = sc.PATCHES[name]
    owner, valid, p = sm.route(patches, shape, ratio)
    sweep = sm.flood_sweep(p["a"], p["second"], p["diff"], p["label"], p["group"])
    assert np.array_equal(sweep, p["flooded"])
    _, alpha, _, _ = sm.stack(patches, shape)
    owned = owner >= 0
    got = np.take_along_axis(alpha, np.maximum(owner, 0).astype(np.int64)[None], axis=0)[0]
    assert (got[owned] > 0).all() and not (owner[~valid] >= 0).any()
    assert p["open"].any() and (owner != p["a"]).any()
    assert (p["label"] == sm.WALL).any()
    # the cases hold what they are for
    covered = sm.stack(patches, shape)[0].sum(axis=0)
    print(name, "open", int(p["open"].sum()), "moved", int((owner != p["a"]).sum()),
          "groups", p["n_groups"], "most cameras on a pixel", int(covered.max()))
    if name.startswith("4-"):
        assert covered.max() == 4 and ratio == 1.0


def test_ghost_pair_seam_lies_on_the_background():
    patches, shape, ratio = sc.ghost_pair()
    owner, valid, p = sm.route(patches, shape, ratio)
    assert valid.all() and p["n_groups"] == 2
    assert (p["diff"] > 0).sum() == 30 * 6              # the rectangle, nothing else
    cols = np.nonzero(p["open"].any(axis=0))[0]
    assert cols.min() < 72 - 3 and cols.max() > 78 + 3  # well inside the zone
    assert not p["diff"][sm.seam_pairs(owner)].any()
    assert p["diff"][sm.seam_pairs(p["a"])].any()       # the argmax seam crosses it
    assert len(set(owner[p["diff"] > 0].tolist())) == 1


def test_binding_declares_the_route_entry_points():
    from pano360_amd import _lib, stitcher
    header = open(f"{ROOT}/include/pano360.h").read()
    for name in ("pano_seam_route_prepare", "pano_seam_route_flood", "pano_seam_route"):
        assert name in _lib.EXPORTS and re.search(rf"\nint {name}\(pano_ctx \*ctx,", header)
    assert stitcher.BLENDERS["seam"] is stitcher.seam_blend
    assert stitcher.SEAM_RATIO == 0.5 and stitcher.seam_blend not in stitcher._FUSED
    assert stitcher.seam_blend.__defaults__ == (5, None)
    assert sc.BATCH == int(re.search(r"#define PANO_SEAM_BATCH (\d+)", header).group(1))


def test_command_line():
    from pano360_amd import stitcher
    args = stitcher.parse_args(["dir", "-b", "seam"])
    assert args.blend == "seam" and not hasattr(args, "seam_ratio")
    assert stitcher.parse_args(["dir", "-b", "seam", "--seam-ratio", "0.25"]).seam_ratio == 0.25
    assert stitcher.parse_args(["dir", "--blend", "seam", "--seam-ratio", "1"]).seam_ratio == 1
    for bad in (["dir", "--seam-ratio", "0.5"], ["dir", "-b", "multiband", "--seam-ratio", "0.5"],
                ["dir", "-b", "seam", "--seam-ratio", "0"], ["dir", "-b", "seam", "--seam-ratio", "1.5"],
                ["dir", "-b", "seam", "--seam-ratio", "nan"]):
        with pytest.raises(SystemExit):
            stitcher.parse_args(bad)
    # no cache name changes
    assert stitcher.cache_name(args) == stitcher.cache_name(stitcher.parse_args(["dir"]))


def test_namespace_without_the_flag_is_what_it_was():
    from pano360_amd import stitcher
    assert vars(stitcher.parse_args(["dir"])) == {
        "path": "dir", "shrink": 2, "ba": "incr", "equalize": False, "crop": False,
        "blend": "multiband", "ghost_tol": None, "out": None, "register": False,
        "detector": "sift", "view": [], "equirect": None, "cube": None, "deepzoom": False,
        "multires": None, "tile": 512, "fill": False, "lens": None, "lens_interp": None,
        "lens_focal": None}
    got = vars(stitcher.parse_args(["dir", "-b", "median", "-c", "-o", "x.jpg"]))
    assert got["blend"] == "median" and "seam_ratio" not in got and len(got) == 20
