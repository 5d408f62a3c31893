"""CPU: the forged level grids of tests/seam_forge.py are what they claim to be.  On every case the
class sweep equals the reference's heap loop; the valley grids and the right-entry serpentines
give both colours a large share (a leak of either colour shows), the valleys put label changes
on the 64-cell borders, and three deliberately wrong floods - written here as variants of
``graph_cut_model.flood_sweep`` - differ from the heap loop on every valley grid, so a device
flood with one of those faults cannot pass tests/test_gpu_seam_forge.py."""
import numpy as np
import pytest
from scipy import ndimage

import graph_cut_model as gm
import seam_forge as sf

VALLEYS_2D = tuple(n for n in sf.NAMES if sf.KIND[n] == "valley" and sf.CASES[n][0].shape[0] >= 2)
# Both colours must own a tenth of the grid: every valley and every right-entry serpentine.  The
# left-entry serpentines are their mirrors, where -1 rightly takes the corridor and then every
# wall (0.997 of the grid); the long rows have one colour's run by construction; the minimal
# grids have at most a handful of free cells.  Those are exempt.
SHARED = tuple(n for n in sf.NAMES if sf.KIND[n] in ("valley", "serpentine-right"))


def wrong_sweep(level, border, eight=False, plus_first=False, strict=False):
    """``flood_sweep`` with one fault: 8-connected components, colour +1 before -1, or a class
    that opens ``level > d`` in place of ``level >= d``."""
    lab = gm.presets(*level.shape, border)
    for d in np.unique(level)[::-1]:
        free = (lab == 0) & ((level > d) if strict else (level >= d))
        if not free.any():
            continue
        comp, n = ndimage.label(free, structure=np.ones((3, 3), int) if eight else None)
        for colour in ((1, -1) if plus_first else (-1, 1)):
            ids = np.zeros(n + 1, bool)
            ids[comp[gm._touching(lab, colour) & (lab == 0) & free]] = True
            ids[0] = False
            lab[ids[comp] & (lab == 0)] = colour
    return lab


def test_the_table_holds_the_listed_cases():
    shapes = {name: (sf.CASES[name][0].shape, sf.CASES[name][1]) for name in sf.NAMES}
    assert len(sf.NAMES) == 21
    assert len(VALLEYS_2D) == 8 and len(SHARED) == 12
    assert shapes["valley-270x290"] == ((270, 290), 14)
    assert shapes["valley-63x127"] == ((63, 127), 5)
    assert shapes["serpentine-left-700x110"] == ((700, 110), 3)
    assert shapes["row-from-right"] == ((1, 27000), 2) and shapes["minimal-1x5"] == ((1, 5), 2)
    assert max(level.size for level, _, _ in sf.CASES.values()) == 300 * 330
    for level, border, _ in sf.CASES.values():
        assert level.dtype == np.int16 and level.min() >= -1 and level.max() <= 255
    # lines longer than one 256-cell group on the resident path, in rows and in columns
    resident = [sf.CASES[n][0].shape for n in sf.NAMES if sf.RESIDENT in sf.CASES[n][2]]
    assert max(s[1] for s in resident) == 27000 and max(s[0] for s in resident) == 2600
    assert (sf.CASES["valley-holes-129x321"][0] == -1).mean() > 0.03
    assert len(np.unique(sf.CASES["valley-step64-200x390"][0])) <= 8


@pytest.mark.parametrize("name", sf.NAMES)
def test_paths_follow_the_resident_size_rule(name):
    from pano360_amd import _lib
    level, border, paths = sf.CASES[name]
    rows, cols = level.shape
    assert sf.RESIDENT_CELLS == _lib.SEAM_RESIDENT_CELLS
    fits = (rows + 2) * (cols + 2) <= _lib.SEAM_RESIDENT_CELLS
    assert sf.TILED in paths and set(paths) <= {sf.RESIDENT, sf.TILED}
    if sf.RESIDENT in paths:
        assert fits
    if not fits:
        assert paths == (sf.TILED,)
    if "300x330" not in name:                       # the two cases kept off the resident path
        assert (sf.RESIDENT in paths) == fits


@pytest.mark.parametrize("name", sf.NAMES)
def test_sweep_equals_heap(name):
    level, border, _ = sf.CASES[name]
    heap, worked = sf.truth(name)                   # asserts sweep == heap
    assert heap.dtype == np.int8 and heap.shape == level.shape
    assert not (heap == 0).any()
    share = float(np.mean(heap == -1))
    print(f"{name}: {level.shape} border {border}: share of -1 {share:.3f}, "
          f"classes that worked {worked}, border pairs {sf.border_pairs(heap)}")
    if name == "minimal-1x5":
        assert worked == 0 and np.array_equal(heap, gm.presets(1, 5, 2))
    if name in SHARED:
        assert min(share, 1 - share) >= 0.10, share
    if name in VALLEYS_2D:
        assert sf.border_pairs(heap) >= 8


def test_the_serpentines_and_rows_are_one_run():
    """The left-entry serpentine hands -1 the corridor and then every wall; its mirror hands +1
    the corridor; the rows are single runs of one colour."""
    heap, worked = sf.truth("serpentine-left-110x700")
    assert np.mean(heap == -1) > 0.99 and worked == 2
    for name in ("serpentine-right-110x700", "serpentine-right-300x330",
                 "serpentine-vertical-right-2600x29"):
        level, border, _ = sf.CASES[name]
        heap, worked = sf.truth(name)
        free = np.ones(level.shape, bool)
        free[:, :border + 1] = False
        free[:, level.shape[1] - border:] = False
        assert (heap[free & (level == 255)] == 1).all()
        if "vertical" in name:                      # its walls lie between +1 corridors
            assert worked == 3
        else:
            assert (heap[free & (level == 0)] == -1).all() and worked == 2
    heap, _ = sf.truth("serpentine-vertical-left-2600x29")
    assert (heap[sf.CASES["serpentine-vertical-left-2600x29"][0] == 255] == -1).all()
    assert (sf.truth("row-from-left")[0][0, :26998] == -1).all()
    assert (sf.truth("row-from-right")[0][0, 4:] == 1).all()
    both = sf.truth("row-both")[0][0]
    cut = 27000 // 2 + 37
    assert (both[:cut + 1] == -1).all() and (both[cut + 1:] == 1).all()


@pytest.mark.parametrize("fault", ("eight", "plus_first", "strict"))
@pytest.mark.parametrize("name", VALLEYS_2D)
def test_wrong_floods_differ_from_the_heap(name, fault):
    level, border, _ = sf.CASES[name]
    heap, _ = sf.truth(name)
    assert np.array_equal(wrong_sweep(level, border), heap)         # the variant without a fault
    wrong = wrong_sweep(level, border, **{fault: True})
    differ = int((wrong != heap).sum())
    print(f"{name}, {fault}: {differ} cells differ")
    assert differ > 0
