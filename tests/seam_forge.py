"""Seeded level grids forged for the seam flood (csrc/graphcut.hip, ``pano_seam_flood``), NumPy
only: the inputs of tests/test_seam_forge_host.py (CPU) and tests/test_gpu_seam_forge.py.

Image-like grids leave most of the flood's machinery idle: lines shorter than one 256-cell group,
walls that never sit on a 64-cell chunk, group or tile border, and colour -1 owning nearly
everything, which hides a leak of -1.  The grids here are built the other way round.

``valley``      levels high at both preset bands and low along a wavy line between them, so the
                two colours meet in the valley and both own a large share; a share of the cells
                dropped to level 0 (tortuous, percolation-like components); and *pickets*: in every
                line the cells ``64 k - 1`` and ``64 k`` are walls (level 0 .. 2) with a given
                probability, which puts walls and run ends exactly on the 64- and 256-cell borders
                of both axes.
``serpentine``  one corridor of level 255 between walls of level 0 that winds through the whole
                grid and is open to one band only: a single class has to carry one colour along
                the whole corridor, across every chunk, group and tile border, in both directions.
long rows       1 x 27000: 106 groups of the resident path, 422 tiles of the tiled one.

``CASES`` maps a name to ``(int16 level grid, border, paths)``; ``paths`` is the subset of
{1 (resident), 2 (tiled)} the grid admits - path 0 (by size) always runs as well.  ``KIND`` maps
the name to its generator.  ``truth`` is the reference's heap loop on a case, computed once."""
import functools

import numpy as np

import graph_cut_model as gm

RESIDENT, TILED = 1, 2
RESIDENT_CELLS = 81408              # PANO_SEAM_RESIDENT_CELLS (include/pano360.h)
BATCH = 64                          # PANO_SEAM_BATCH
CHUNK = 64                          # cells per ballot; four of them make a resident group


def marks(n):
    """The cells on either side of every 64-cell border of a line of ``n`` cells."""
    return [m for k in range(1, n // CHUNK + 1) for m in (CHUNK * k - 1, CHUNK * k) if m < n]


def valley(rows, cols, seed, drop=0.35, picket=0.5, holes=0.0, step=1):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:rows, :cols].astype(np.float64)
    phase = rng.uniform(0, 2 * np.pi)
    centre = cols * (0.5 + 0.2 * np.sin(2 * np.pi * 1.5 * y / rows + phase))
    level = 20 + 200 * np.abs(x - centre) / (cols / 2)
    level = np.floor(level).astype(np.int64) + rng.integers(-30, 31, (rows, cols))
    level = np.clip(level, 3, 255) // step * step
    level[rng.random((rows, cols)) < drop] = 0
    for m in marks(cols):                           # in every row, each mark column
        hit = rng.random(rows) < picket
        level[hit, m] = rng.integers(0, 3, int(hit.sum()))
    for m in marks(rows):                           # in every column, each mark row
        hit = rng.random(cols) < picket
        level[m, hit] = rng.integers(0, 3, int(hit.sum()))
    if holes:
        level[rng.random((rows, cols)) < holes] = -1
    return level.astype(np.int16)


def serpentine(rows, cols, border, pitch, enter, vertical=False):
    """Walls of level 0; corridors of level 255 every ``pitch`` rows over the columns
    ``border + 2 .. cols - border - 3``, joined at alternating ends into one path.  The door - the
    cells of row 0 between the first corridor and a band: column ``border + 1`` on the left,
    ``cols - border - 2`` and ``cols - border - 1`` on the right - opens that end of the path, and
    the first joint is at the other end, so the colour that enters walks every corridor.
    ``vertical``: corridors every ``pitch`` columns over all rows instead, the door at the free
    end of the first (left) or last (right) corridor."""
    level = np.zeros((rows, cols), np.int16)
    lo, hi = border + 2, cols - border - 3
    assert enter in ("left", "right") and lo < hi
    if vertical:
        xs = list(range(lo, hi + 1, pitch))
        for k, x in enumerate(xs):
            level[:, x] = 255
            if k + 1 < len(xs):                     # the first joint is at the bottom
                level[rows - 1 if k % 2 == 0 else 0, x:xs[k + 1]] = 255
        if enter == "left":
            level[0, border + 1:lo] = 255
        else:
            level[0 if len(xs) % 2 == 0 else rows - 1, xs[-1]:cols - border] = 255
        return level
    far = hi if enter == "left" else lo
    near = lo if enter == "left" else hi
    ys = list(range(0, rows, pitch))
    for k, y in enumerate(ys):
        level[y, lo:hi + 1] = 255
        if k + 1 < len(ys):
            level[y:ys[k + 1], far if k % 2 == 0 else near] = 255
    if enter == "left":
        level[0, border + 1:lo] = 255
    else:
        level[0, hi + 1:cols - border] = 255
    return level


def long_row(kind, cols=27000):
    level = np.full((1, cols), 255, np.int16)
    if kind == "right":                             # only +1 can enter, and has to travel left
        level[0, 3] = 0
    elif kind == "both":
        level[0, cols // 2 + 37] = 0
    return level


def _paths(level, want=(RESIDENT, TILED)):
    rows, cols = level.shape
    fits = (rows + 2) * (cols + 2) <= RESIDENT_CELLS
    return tuple(p for p in want if p != RESIDENT or fits)


CASES, KIND = {}, {}


def _add(name, kind, level, border, want=(RESIDENT, TILED)):
    assert name not in CASES and level.dtype == np.int16
    CASES[name] = (level, border, _paths(level, want))
    KIND[name] = kind


def _valley(rows, cols, border, tag="", want=(RESIDENT, TILED), **kw):
    _add(f"valley{tag}-{rows}x{cols}", "valley", valley(rows, cols, rows + cols, **kw), border,
         want)


_valley(110, 700, 2)
_valley(270, 290, 14)
_valley(2600, 29, 2)
_valley(129, 321, 3, "-holes", holes=0.05)
_valley(200, 390, 2, "-step64", step=64)
_valley(300, 330, 2, want=(TILED,))
_valley(1, 27000, 2, "-row", drop=0.0, picket=0.02)
_valley(65, 129, 2)
_valley(63, 127, 5)
for _enter in ("left", "right"):
    _add(f"serpentine-{_enter}-110x700", f"serpentine-{_enter}",
         serpentine(110, 700, 2, 2, _enter), 2)
_add("serpentine-left-700x110", "serpentine-left", serpentine(700, 110, 3, 2, "left"), 3)
_add("serpentine-right-300x330", "serpentine-right", serpentine(300, 330, 2, 2, "right"), 2,
     (TILED,))
for _enter in ("left", "right"):
    _add(f"serpentine-vertical-{_enter}-2600x29", f"serpentine-{_enter}",
         serpentine(2600, 29, 2, 2, _enter, vertical=True), 2)
for _kind in ("left", "right", "both"):
    _add(f"row-from-{_kind}" if _kind != "both" else "row-both", "row", long_row(_kind), 2)
for _rows, _cols in ((1, 5), (1, 6), (3, 6)):       # 1 x 5 is all preset: nothing floods
    _add(f"minimal-{_rows}x{_cols}", "minimal",
         np.random.default_rng(_rows + _cols).integers(0, 4, (_rows, _cols)).astype(np.int16), 2)

NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def truth(name):
    """(the heap loop's labels, the classes that labelled a cell in the sweep), read-only."""
    level, border, _ = CASES[name]
    heap = gm.flood_heap(level, border)
    sweep, worked = gm.flood_sweep(level, border, want_stats=True)
    assert np.array_equal(sweep, heap), name
    heap.setflags(write=False)
    return heap, worked


def border_pairs(lab):
    """Pairs of 4-neighbours on opposite sides of a 64-cell border (either axis) whose labels
    differ."""
    rows, cols = lab.shape
    n = 0
    for k in range(CHUNK, cols, CHUNK):
        n += int((lab[:, k - 1] != lab[:, k]).sum())
    for k in range(CHUNK, rows, CHUNK):
        n += int((lab[k - 1] != lab[k]).sum())
    return n
