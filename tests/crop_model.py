"""The contract of ``pano_crop_rect`` (csrc/crop.hip) by definition, in NumPy integers.

``heights[i][j]`` is the length of the upward run of non-zero pixels that ends at (i, j).  For a
bottom row ``i`` and a column ``j`` with ``h = heights[i][j] > 0`` the candidate rectangle is the
maximal run of columns around ``j`` whose heights in row ``i`` are ``>= h``, ``h`` rows high.
Column 0 is the exception: its right extent is always 0, so its candidate is one pixel wide.  The
winner is the first candidate in (row ascending, column ascending) order whose area is strictly
larger than that of every candidate before it.

Nothing here is shared with the two implementations under test: no monotonic stack (the
oracle's nearest-smaller search) and no chunk minima (the kernel's).  Per row and per distinct
height ``h`` of that row the runs of ``row >= h`` are read off ``np.diff`` and every column of
height ``h`` takes the run it lies in.  Python loops go over rows and over the distinct heights of
a row, never over pixels.
"""
from collections import namedtuple

import numpy as np

# rect = (y0, x0, h, w); (i, j) = the bottom row and the column whose candidate won
Winner = namedtuple("Winner", "rect area i j")


def heights(mask):
    """int32 [H][W]: the number of non-zero pixels straight up from (i, j), itself included, before
    the first zero."""
    mask = np.asarray(mask)
    H, W = mask.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    last_zero = np.maximum.accumulate(np.where(mask != 0, -1, rows), axis=0)   # -1: none so far
    return (rows - last_zero).astype(np.int32)


def _row_extents(row):
    """(left, right), inclusive, of the maximal run of ``row >= row[j]`` around every column j
    (columns of height 0: left = right = j, never read)."""
    W = len(row)
    left = np.arange(W, dtype=np.int64)
    right = left.copy()
    for h in np.unique(row[row > 0]):
        edge = np.diff(np.concatenate(([0], (row >= h).astype(np.int8), [0])))
        start = np.flatnonzero(edge == 1)                   # first column of each run
        stop = np.flatnonzero(edge == -1) - 1               # last column of each run
        run_of = np.cumsum(edge[:-1] == 1) - 1              # index of the run a column lies in
        cols = np.flatnonzero(row == h)
        left[cols] = start[run_of[cols]]
        right[cols] = stop[run_of[cols]]
    return left, right


def candidates(mask, quirk=True):
    """(heights, left, right, area), each [H][W]: the candidate of every (bottom row, column);
    area 0 where the height is 0.  ``quirk=False``: column 0 like every other column."""
    hgt = heights(mask)
    left = np.empty(hgt.shape, np.int64)
    right = np.empty(hgt.shape, np.int64)
    for i in range(hgt.shape[0]):
        left[i], right[i] = _row_extents(hgt[i])
    if quirk:
        right[:, 0] = 0
    area = (right - left + 1) * hgt.astype(np.int64)
    return hgt, left, right, area


def search(mask, quirk=True):
    """The ``Winner``, or None for a mask without a non-zero pixel."""
    hgt, left, right, area = candidates(mask, quirk)
    if not area.any():
        return None
    # the first candidate strictly larger than all before it, in row-major order, is the first
    # occurrence of the largest area: np.argmax returns the first of equal maxima
    i, j = np.unravel_index(int(np.argmax(area.ravel())), area.shape)
    h, l, r = int(hgt[i, j]), int(left[i, j]), int(right[i, j])
    return Winner((int(i) - h + 1, l, h, r - l + 1), int(area[i, j]), int(i), int(j))


def crop_rect(mask, quirk=True):
    """((y0, x0, h, w), area), or None for an empty mask."""
    win = search(mask, quirk)
    return None if win is None else (win.rect, win.area)
