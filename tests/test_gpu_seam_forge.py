"""GPU: ``pano_seam_flood`` (csrc/graphcut.hip) on the forged level grids of tests/seam_forge.py,
handed to ``blend.seam_flood_device`` directly, against the reference's heap loop
(``graph_cut_model.flood_heap``).  Labels are integers and every comparison is equality.

What the grids reach that image-like inputs leave idle (tests/test_seam_forge_host.py shows on
the CPU that they are sharp): resident lines of up to 106 groups of 256 cells - both directions
of ``seam_line_pass<4>``, the carry between groups, the frame cell behind the last group -, walls
and run ends on the 64- and 256-cell borders of both axes, tiles whose neighbours write while
they load their halo, classes that need hundreds of rounds so that the host's read of "done"
lands inside a class, and the count of classes that labelled a cell (``stats[0]``)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import graph_cut_model as gm  # noqa: E402
import seam_forge as sf  # noqa: E402

pytestmark = pytest.mark.gpu


def flood(eng, level, border, path):
    """(labels, stats) of one call as host arrays."""
    import torch
    from pano360_amd import blend
    labels, stats = blend.seam_flood_device(torch.from_numpy(level).to(eng.device), border, eng,
                                            path, want_stats=True)
    return labels.cpu().numpy(), stats.cpu().numpy()


def assert_labels(got, want, what):
    assert got.dtype == np.int8 and got.shape == want.shape, what
    wrong = np.argwhere(got != want)
    if len(wrong):
        first = [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in wrong[:12]]
        print(f"{what}: {len(wrong)} cells differ; first (row, col, got, want): {first}")
    assert len(wrong) == 0, what


@pytest.mark.parametrize("name", sf.NAMES)
def test_labels_and_classes_equal_the_heap_loop(eng, name):
    """Path 0 and every path the grid admits: every label, the number of classes that labelled
    a cell, the path taken, and the same bytes from a second run."""
    level, border, paths = sf.CASES[name]
    want, worked = sf.truth(name)
    rows, cols = level.shape
    by_size = sf.RESIDENT if (rows + 2) * (cols + 2) <= sf.RESIDENT_CELLS else sf.TILED
    seen = {}
    for path in (0,) + paths:
        labels, stats = flood(eng, level, border, path)
        taken = path or by_size
        print(f"{name} {level.shape} path {path}: classes {stats[0]} (sweep {worked}), "
              f"{'passes' if taken == sf.RESIDENT else 'rounds'} {stats[1]}, "
              f"most in one class {stats[2]}")
        assert_labels(labels, want, f"{name}, path {path}")
        assert int(stats[3]) == taken
        assert int(stats[0]) == worked
        again, stats2 = flood(eng, level, border, path)
        assert labels.tobytes() == again.tobytes() and int(stats2[0]) == worked
        seen[taken] = labels
    if len(seen) == 2:
        assert np.array_equal(seen[sf.RESIDENT], seen[sf.TILED])


def test_random_small_grids_on_both_paths(eng):
    """The 120 grids of test_graph_cut_host.test_sweep_equals_heap_on_random_grids, same seed."""
    from test_graph_cut_host import random_level_grid
    rng = np.random.default_rng(20260)
    for k in range(120):
        level, border = random_level_grid(rng)
        want = gm.flood_heap(level, border)
        for path in (sf.RESIDENT, sf.TILED):
            labels, stats = flood(eng, level, border, path)
            assert_labels(labels, want, f"grid {k} {level.shape} border {border}, path {path}")
            assert int(stats[3]) == path


@pytest.mark.parametrize("name", ("serpentine-right-300x330", "row-from-right"))
def test_one_class_outlasts_a_batch_of_rounds(eng, name):
    """Tiled path: class (255, +1) needs more rounds than the host queues between two reads of
    "done" (PANO_SEAM_BATCH = 64), so a read lands inside the class.  The count is the device's
    own (``stats[2]``) and depends on when tiles load their halos.  Measured on one MI355X: the
    serpentine 770 rounds, 755 of them in that class (150 corridors across six tiles each); the
    row 423 rounds, 422 in that class (one tile of the 422 per round)."""
    level, border, _ = sf.CASES[name]
    labels, stats = flood(eng, level, border, sf.TILED)
    print(f"{name}: {stats[1]} rounds, {stats[2]} in one class")
    assert int(stats[2]) > sf.BATCH
    assert_labels(labels, sf.truth(name)[0], name)


def test_one_engine_small_large_small_then_resident(eng):
    """A fresh engine's seam state and scratch: a small tiled flood, the largest tiled case, the
    small one again with identical bytes, then a resident flood."""
    from pano360_amd import engine
    use = engine.Engine(eng.device)
    small, large, resident = "valley-63x127", "valley-300x330", "valley-65x129"
    assert sf.CASES[large][0].size == max(level.size for level, _, _ in sf.CASES.values())
    first, stats = flood(use, *sf.CASES[small][:2], sf.TILED)
    assert_labels(first, sf.truth(small)[0], small)
    big, _ = flood(use, *sf.CASES[large][:2], sf.TILED)
    assert_labels(big, sf.truth(large)[0], large)
    again, stats2 = flood(use, *sf.CASES[small][:2], sf.TILED)
    assert first.tobytes() == again.tobytes() and int(stats[0]) == int(stats2[0])
    labels, stats = flood(use, *sf.CASES[resident][:2], sf.RESIDENT)
    assert_labels(labels, sf.truth(resident)[0], resident)
    assert int(stats[0]) == sf.truth(resident)[1] and int(stats[3]) == sf.RESIDENT
