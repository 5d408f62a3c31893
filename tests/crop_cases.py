"""Forged valid masks for ``pano_crop_rect`` (csrc/crop.hip): ``CASES`` maps a name to a uint8
[H][W] mask, built once at import, deterministic, none above 12 x 8300 pixels.  The groups below
(``QUIRK``, ``TIES``, ``EDGES``, ``FINALISE``, ``HEIGHTS``, ``SKYLINES`` ...) name the cases of
one family; what each family claims about its masks is asserted on the model alone in
tests/test_crop_host.py.

The kernel's geometry the sizes are placed around: the heights scan gives each column's rows to
16 segments of ceil(H / 16) rows; the row search keeps minima of 64-column chunks and of
64-chunk (4096-column) super-chunks, gives 2048 columns of a row to a workgroup and, inside it,
64 consecutive columns to a wave; the finalise step walks 64 columns per ballot.
"""
import numpy as np

CASES = {}


def _add(name, mask):
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    assert name not in CASES and mask.ndim == 2 and 0 < mask.size <= 200_000, name
    mask.setflags(write=False)
    CASES[name] = mask
    return name


def from_heights(H, bottom):
    """The mask of H rows whose column j is valid in its lowest ``bottom[j]`` rows."""
    bottom = np.asarray(bottom)
    return (np.arange(H)[:, None] >= H - bottom[None, :]).astype(np.uint8)


# ------------------------------------------------------------------------------------- quirk
# Column 0 is the only column shorter than the rest, by one pixel, and H > W: the natural
# definition takes the full width at height H - 1 (W (H - 1) > (W - 1) H), the contract cannot
# (column 0's candidate is one pixel wide) and takes columns 1 .. W - 1 at height H.
def _col0_short(H, W):
    mask = np.ones((H, W), np.uint8)
    mask[0, 0] = 0
    return mask


def _only_col0(H, W):
    mask = np.zeros((H, W), np.uint8)
    mask[:, 0] = 1
    return mask


def _one_wide(H, hole):
    mask = np.ones((H, 1), np.uint8)
    mask[hole, 0] = 0
    return mask


QUIRK_CHANGES_RECT = [_add("quirk_col0_short_5x4", _col0_short(5, 4)),
                      _add("quirk_col0_short_70x65", _col0_short(70, 65))]
QUIRK_ONLY_COL0 = [_add("quirk_only_col0_6x70", _only_col0(6, 70)),
                   _add("quirk_one_wide_7x1", _one_wide(7, 2)),
                   _add("quirk_one_pixel", np.ones((1, 1), np.uint8))]
QUIRK_ALL_VALID = [_add("quirk_all_valid_5x5", np.ones((5, 5), np.uint8))]
QUIRK = QUIRK_CHANGES_RECT + QUIRK_ONLY_COL0 + QUIRK_ALL_VALID


# -------------------------------------------------------------------------------------- ties
# name -> ((rect, area) first in scan order, (rect, area) later in scan order); rect = (y0, x0, h, w)
TIES = {}


def _upper_lower(H, W, upper_rows, x0, w):
    """Rows [0, upper_rows) all valid, one empty row, the rest valid over columns [x0, x0 + w)."""
    mask = np.zeros((H, W), np.uint8)
    mask[:upper_rows] = 1
    mask[upper_rows + 1:, x0:x0 + w] = 1
    lower_rows = H - upper_rows - 1
    return mask, (((0, 0, upper_rows, W), upper_rows * W),
                  ((upper_rows + 1, x0, lower_rows, w), lower_rows * w))


def _two_runs(H, W, a, b, w):
    mask = np.zeros((H, W), np.uint8)
    mask[:, a:a + w] = 1
    mask[:, b:b + w] = 1
    return mask, (((0, a, H, w), H * w), ((0, b, H, w), H * w))


def _tie(name, built):
    TIES[_add(name, built[0])] = built[1]
    return name


# 3 x 64 = 4 x 48 = 192; 2 x 4224 = 3 x 2816 = 8448 (the lower one spans workgroups 0 .. 1)
TIE_UPPER_WINS = [_tie("tie_upper_lower_8x64", _upper_lower(8, 64, 3, 5, 48)),
                  _tie("tie_upper_lower_6x4224", _upper_lower(6, 4224, 2, 700, 2816))]
# 3 x 65 = 195 against 4 x 49 = 196
TIE_LOWER_WINS = [_tie("tie_lower_larger_by_one_8x65", _upper_lower(8, 65, 3, 5, 49))]
# columns 10 .. 109 and 3000 .. 3099: workgroups 0 and 1;  10 .. 39 and 140 .. 169: waves 0 and 2
TIE_LEFT_WINS = [_tie("tie_two_runs_two_workgroups_3x4500", _two_runs(3, 4500, 10, 3000, 100)),
                 _tie("tie_two_runs_two_waves_3x256", _two_runs(3, 256, 10, 140, 30))]
TIE_FIRST_WINS = TIE_UPPER_WINS + TIE_LEFT_WINS


# --------------------------------------------------- chunk, super-chunk and segment edges
EDGE_WIDTHS = {64: 12, 65: 7, 2048: 5, 2049: 3, 4096: 4, 4097: 6, 8192: 2, 8193: 9, 8300: 12}
NOTCH_COLUMNS = (63, 64, 4095, 4096)
STAIR_H = STAIR_STEPS = 12
EDGES, STAIRS = [], []


def _notched(H, W, cols):
    """All valid but the top max(1, H // 2) rows of ``cols``: their heights are 0 there and
    positive but lower than their neighbours' below."""
    mask = np.ones((H, W), np.uint8)
    mask[:max(1, H // 2), cols] = 0
    return mask


def staircase(W, rising=True):
    """12 steps of equal width, heights 1 .. 12 to the right (or to the left), 12 rows."""
    step = np.arange(W) * STAIR_STEPS // W + 1
    return from_heights(STAIR_H, step if rising else step[::-1])


for _W, _H in EDGE_WIDTHS.items():
    EDGES.append(_add(f"edge_all_valid_{_H}x{_W}", np.ones((_H, _W), np.uint8)))
    for _c in sorted({c for c in NOTCH_COLUMNS if c < _W} | {_W - 1}):
        EDGES.append(_add(f"edge_notch_at_{_c}_{_H}x{_W}", _notched(_H, _W, [_c])))
    EDGES.append(_add(f"edge_notch_every_64th_from_63_{_H}x{_W}",
                      _notched(_H, _W, np.arange(63, _W, 64))))
    if _W > 64:
        EDGES.append(_add(f"edge_notch_every_64th_from_64_{_H}x{_W}",
                          _notched(_H, _W, np.arange(64, _W, 64))))
    _rng = np.random.default_rng(1000 + _W)
    _holes = np.ones((_H, _W), np.uint8)
    _holes[_rng.integers(0, _H, 5), _rng.integers(0, _W, 5)] = 0
    EDGES.append(_add(f"edge_five_holes_{_H}x{_W}", _holes))
    # one column lower than all others inside the last chunk (the partial one where W % 64 != 0)
    _last = (_W - 1) // 64 * 64
    _low = np.full(_W, _H)
    _low[_last + (_W - 1 - _last) // 2] = 1
    EDGES.append(_add(f"edge_low_column_in_last_chunk_{_H}x{_W}", from_heights(_H, _low)))
    STAIRS.append(_add(f"stairs_rising_{STAIR_H}x{_W}", staircase(_W, True)))
    STAIRS.append(_add(f"stairs_falling_{STAIR_H}x{_W}", staircase(_W, False)))
EDGES += STAIRS


# ---------------------------------------------------------------------------------- finalise
# name -> (columns left of the winner's first column, columns right of it)
FINALISE = {}


def _wings(left, right, margin_left, margin_right):
    """4 rows.  ``left`` columns of height 4, then 1 + ``right`` columns of height 3: the widest
    candidate, 3 x (left + 1 + right), first appears at the first column of height 3 and has
    ``left`` columns on its left (3 (left + 1 + right) > 4 left for the sizes used)."""
    assert 3 * (left + 1 + right) > 4 * left
    bottom = np.concatenate((np.zeros(margin_left, int), np.full(left, 4),
                             np.full(1 + right, 3), np.zeros(margin_right, int)))
    return from_heights(4, bottom)


for _l, _r in ((63, 63), (64, 64), (65, 65), (128, 128), (63, 128), (128, 63)):
    FINALISE[_add(f"finalise_{_l}_left_{_r}_right", _wings(_l, _r, 3, 2))] = (_l, _r)
FINALISE[_add("finalise_reaches_column_0", _wings(64, 65, 0, 2))] = (64, 65)
FINALISE[_add("finalise_reaches_last_column", _wings(65, 64, 3, 0))] = (65, 64)
FINALISE[_add("finalise_reaches_both_ends", _wings(128, 129, 0, 0))] = (128, 129)


# ------------------------------------------------------------------------------ heights scan
SCAN_HEIGHTS = (1, 15, 16, 17, 31, 32, 33, 47)
SCAN_W = 70            # two blocks of 64 columns, the second partial
HEIGHTS = []


def _scan_runs(H, W):
    """Column x: valid from row ``start`` in segment x % 13 up to a row three segments further
    down, invalid at ``start - 1`` and valid above that (a run that must not leak across the
    gap); odd columns are valid again below the end of the run."""
    hs = (H + 15) // 16
    mask = np.zeros((H, W), np.uint8)
    for x in range(W):
        start = min((x % 13) * hs + x % hs, H - 1)
        end = min(start + 3 * hs + 1, H)                        # one past the run's last row
        mask[:max(start - 1, 0), x] = 1
        mask[start:end, x] = 1
        if x % 2:
            mask[end + 1:, x] = 1
    return mask


def _last_row_off(H, W):
    mask = np.ones((H, W), np.uint8)
    mask[H - 1, ::3] = 0
    return mask


for _H in SCAN_HEIGHTS:
    HEIGHTS.append(_add(f"scan_valid_throughout_{_H}x{SCAN_W}", np.ones((_H, SCAN_W), np.uint8)))
    HEIGHTS.append(_add(f"scan_runs_over_three_segments_{_H}x{SCAN_W}", _scan_runs(_H, SCAN_W)))
    HEIGHTS.append(_add(f"scan_last_row_invalid_{_H}x{SCAN_W}", _last_row_off(_H, SCAN_W)))


# --------------------------------------------------------------------------- random skylines
N_SKYLINES = 200
PLATEAU = 37
SKYLINES = []


def skyline(seed, shape=None):
    """At most 8 x 400 from per-column tops, three in ten of them empty columns, so that the
    mask falls into islands that often tie; odd seeds: plateaus of 37 columns; seeds with bit 1
    set: flipped vertically (every run then starts at row 0)."""
    rng = np.random.default_rng(5000 + seed)
    H, W = shape or (int(rng.integers(1, 9)), int(rng.integers(1, 401)))
    n = -(-W // PLATEAU) if seed % 2 else W
    bottom = rng.integers(0, H + 1, n) * (rng.random(n) < 0.7)
    if seed % 2:
        bottom = np.repeat(bottom, PLATEAU)[:W]
    bottom[int(rng.integers(0, W))] = H                 # never empty
    mask = from_heights(H, bottom)
    return mask[::-1] if seed & 2 else mask


for _s in range(N_SKYLINES):
    SKYLINES.append(_add(f"skyline_{_s:03d}", skyline(_s)))


# ------------------------------------------------------------------------------------ values
def _values_2_and_255():
    mask = skyline(1, (8, 300)).astype(np.uint8)
    rng = np.random.default_rng(77)
    return mask * rng.choice(np.array([2, 255], np.uint8), mask.shape)


VALUES = [_add("values_2_and_255", _values_2_and_255())]

EMPTY_SHAPES = ((1, 1), (3, 8300), (40, 70))
