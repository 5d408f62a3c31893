"""CPU: the model of ``pano_crop_rect``'s contract (tests/crop_model.py) against the oracle and the
reference's own rectangles in tests/golden/pure, and the property each family of forged masks in
tests/crop_cases.py claims, evaluated on the model alone.  Integer equality throughout."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_cases as cc  # noqa: E402
import crop_model as cm  # noqa: E402
from conftest import load_golden  # noqa: E402


def test_model_equals_the_oracle_on_every_case(oracle):
    for name, mask in cc.CASES.items():
        rect, area = cm.crop_rect(mask)
        assert rect == oracle.crop_rect(mask), name
        assert area == rect[2] * rect[3] > 0, name
        y0, x0, h, w = rect
        assert mask[y0:y0 + h, x0:x0 + w].all(), name


def test_model_reproduces_the_reference_rectangles():
    g = load_golden("pure")
    n = int(g["n_crop"])
    assert n >= 7
    for k in range(n):
        rect, _ = cm.crop_rect(g[f"crop_mask_{k}"])
        assert rect == tuple(int(v) for v in g[f"crop_rect_{k}"]), k


def test_model_heights_by_the_recurrence():
    """``heights`` against the row-by-row recurrence on cases of every family."""
    for name in cc.HEIGHTS + cc.SKYLINES[:20] + cc.VALUES + ["edge_five_holes_12x8300"]:
        mask = cc.CASES[name]
        want = np.zeros(mask.shape, np.int32)
        run = np.zeros(mask.shape[1], np.int32)
        for i in range(mask.shape[0]):
            run = np.where(mask[i] != 0, run + 1, 0)
            want[i] = run
        got = cm.heights(mask)
        assert got.dtype == np.int32 and np.array_equal(got, want), name


def test_model_is_quick_on_the_widest_case():
    mask = cc.CASES["stairs_rising_12x8300"]
    assert mask.shape == (12, 8300)
    start = time.perf_counter()
    cm.crop_rect(mask)
    assert time.perf_counter() - start < 1.0


def test_empty_mask_has_no_rectangle():
    for shape in cc.EMPTY_SHAPES:
        assert cm.crop_rect(np.zeros(shape, np.uint8)) is None


def test_cases_are_complete_and_small():
    names = (cc.QUIRK + list(cc.TIES) + cc.EDGES + list(cc.FINALISE) + cc.HEIGHTS + cc.SKYLINES
             + cc.VALUES)
    assert sorted(names) == sorted(cc.CASES)                # every case belongs to one family
    for name, mask in cc.CASES.items():
        assert mask.dtype == np.uint8 and mask.flags.c_contiguous and mask.size <= 200_000, name
        assert mask.any(), name
    assert max(m.shape[1] for m in cc.CASES.values()) == 8300
    assert max(m.size for m in cc.CASES.values()) == 12 * 8300


# ------------------------------------------------------------------------------------- quirk
def test_quirk_changes_the_rectangle():
    """Column 0 one pixel short and H > W: without the quirk the full width at height H - 1."""
    assert cm.crop_rect(cc.CASES["quirk_col0_short_5x4"]) == ((0, 1, 5, 3), 15)
    for name in cc.QUIRK_CHANGES_RECT:
        mask = cc.CASES[name]
        H, W = mask.shape
        assert cm.crop_rect(mask) == ((0, 1, H, W - 1), H * (W - 1)), name
        assert cm.crop_rect(mask, quirk=False) == ((1, 0, H - 1, W), (H - 1) * W), name
        assert (H - 1) * W > H * (W - 1)


def test_quirk_cases_whose_winner_is_column_0():
    """Only column 0 holds anything: its one-pixel-wide candidate is the winner, right extent 0."""
    want = {"quirk_only_col0_6x70": (0, 0, 6, 1), "quirk_one_wide_7x1": (3, 0, 4, 1),
            "quirk_one_pixel": (0, 0, 1, 1)}
    assert sorted(want) == sorted(cc.QUIRK_ONLY_COL0)
    for name, rect in want.items():
        win = cm.search(cc.CASES[name])
        assert win.rect == rect and win.j == 0 and win.area == rect[2], name


def test_quirk_moves_the_winner_of_an_all_valid_mask():
    """All valid: the same rectangle with and without the quirk, but column 0's candidate is one
    pixel wide, so the full width is first seen from column 1."""
    for name in cc.QUIRK_ALL_VALID + [n for n in cc.EDGES if n.startswith("edge_all_valid")]:
        mask = cc.CASES[name]
        H, W = mask.shape
        assert mask.all()
        with_quirk, without = cm.search(mask), cm.search(mask, quirk=False)
        assert with_quirk.rect == without.rect == (0, 0, H, W), name
        assert (with_quirk.i, with_quirk.j) == (H - 1, 1) and (without.i, without.j) == (H - 1, 0)
        assert cm.candidates(mask)[3][H - 1, 0] == H


# -------------------------------------------------------------------------------------- ties
def _is_candidate(mask, rect, area):
    """``rect`` is all valid, has ``area`` pixels and is the candidate of one of its columns in
    its bottom row."""
    y0, x0, h, w = rect
    hgt, left, right, cand = cm.candidates(mask)
    i = y0 + h - 1
    cols = np.arange(x0, x0 + w)
    hit = (hgt[i, cols] == h) & (left[i, cols] == x0) & (right[i, cols] == x0 + w - 1)
    return bool(mask[y0:y0 + h, x0:x0 + w].all() and h * w == area and hit.any()
                and (cand[i, cols[hit]] == area).all())


def test_tie_cases_hold_the_areas_they_claim():
    assert sorted(cc.TIES) == sorted(cc.TIE_FIRST_WINS + cc.TIE_LOWER_WINS)
    for name, ((first, area_first), (later, area_later)) in cc.TIES.items():
        mask = cc.CASES[name]
        assert _is_candidate(mask, first, area_first), name
        assert _is_candidate(mask, later, area_later), name
        assert (first[0] + first[2], first[1]) < (later[0] + later[2], later[1])    # scan order
        rect, area = cm.crop_rect(mask)
        if name in cc.TIE_FIRST_WINS:
            assert area_first == area_later and (rect, area) == (first, area_first), name
        else:
            assert area_later == area_first + 1 and (rect, area) == (later, area_later), name
        assert cm.candidates(mask)[3].max() == area                # and nothing else is larger


def test_tie_geometry():
    ties = cc.TIES
    assert ties["tie_upper_lower_8x64"] == (((0, 0, 3, 64), 192), ((4, 5, 4, 48), 192))
    assert ties["tie_lower_larger_by_one_8x65"] == (((0, 0, 3, 65), 195), ((4, 5, 4, 49), 196))
    for name in cc.TIE_UPPER_WINS:
        (first, _), (later, _) = ties[name]
        assert first[1] == 0 and first[3] == cc.CASES[name].shape[1]      # full width, (i + 1) W
        assert first[0] + first[2] < later[0]
    a, b = (ties["tie_two_runs_two_workgroups_3x4500"][k][0][1] for k in (0, 1))
    assert b - a > 2048 and a // 2048 != b // 2048
    a, b = (ties["tie_two_runs_two_waves_3x256"][k][0][1] for k in (0, 1))
    assert a // 256 == b // 256 and a // 64 != b // 64


# ------------------------------------------------------------------------------------- edges
def test_edge_widths_cross_the_chunk_and_super_chunk_sizes():
    assert sorted(cc.EDGE_WIDTHS) == [64, 65, 2048, 2049, 4096, 4097, 8192, 8193, 8300]
    assert all(2 <= h <= 12 for h in cc.EDGE_WIDTHS.values())
    for W, H in cc.EDGE_WIDTHS.items():
        have = [n for n in cc.EDGES if n.endswith(f"x{W}")]
        for c in (63, 64, 4095, 4096, W - 1):
            assert (f"edge_notch_at_{c}_{H}x{W}" in have) == (c < W), (c, W)
        for family in ("edge_all_valid", "edge_notch_every_64th_from_63", "edge_five_holes",
                       "edge_low_column_in_last_chunk"):
            assert f"{family}_{H}x{W}" in have
        assert f"stairs_rising_12x{W}" in have and f"stairs_falling_12x{W}" in have


def test_notches_lie_where_their_names_say():
    for name in cc.EDGES:
        mask = cc.CASES[name]
        H, W = mask.shape
        bottom = cm.heights(mask)[H - 1]
        if name.startswith("edge_notch_at_"):
            c = int(name.split("_")[3])
            low = np.flatnonzero(bottom < H)
            assert low.tolist() == [c] and 0 < bottom[c] < H and cm.heights(mask)[0, c] == 0, name
        elif name.startswith("edge_notch_every_64th_from_"):
            first = int(name.split("_")[5])
            assert np.flatnonzero(bottom < H).tolist() == list(range(first, W, 64)), name
        elif name.startswith("edge_five_holes"):
            assert 1 <= int((mask == 0).sum()) <= 5, name
        elif name.startswith("edge_low_column"):
            low = np.flatnonzero(bottom < H)
            assert len(low) == 1 and low[0] // 64 == (W - 1) // 64 and bottom[low[0]] == 1, name


def test_staircases_have_twelve_long_steps():
    """Equal heights over W / 12 columns, so above 4096 x 12 / 2 columns a step covers whole
    super-chunks; the nearest smaller column of a step's columns is the step boundary on one side
    and absent on the other."""
    for name in cc.STAIRS:
        mask = cc.CASES[name]
        H, W = mask.shape
        bottom = cm.heights(mask)[H - 1].astype(int)
        assert H == 12 and sorted(set(bottom.tolist())) == list(range(1, 13)), name
        step = np.diff(bottom)
        assert np.all(step >= 0) if "rising" in name else np.all(step <= 0), name
        hgt, left, right, _ = cm.candidates(mask)
        edge = np.flatnonzero(step) + 1                     # first columns of steps 2 .. 12
        if "rising" in name:
            assert np.all(right[H - 1, 1:] == W - 1)        # no smaller column on the right
            assert sorted(set(left[H - 1].tolist())) == [0] + edge.tolist()
        else:
            assert np.all(left[H - 1] == 0)
            assert sorted(set(right[H - 1, 1:].tolist())) == (edge - 1).tolist() + [W - 1]
    # the step from height 6 to 7 at, one past and 54 past the super-chunk edge (column 4096)
    for W, first_of_7 in ((8192, 4096), (8193, 4097), (8300, 4150)):
        bottom = cm.heights(cc.CASES[f"stairs_rising_12x{W}"])[11]
        assert np.flatnonzero(bottom == 7)[0] == first_of_7 and bottom[first_of_7 - 1] == 6


# ---------------------------------------------------------------------------------- finalise
def test_finalise_cases_extend_as_far_as_they_claim():
    seen_left, seen_right = set(), set()
    for name, (n_left, n_right) in cc.FINALISE.items():
        mask = cc.CASES[name]
        win = cm.search(mask)
        y0, x0, h, w = win.rect
        assert (win.j - x0, x0 + w - 1 - win.j) == (n_left, n_right), name
        assert (h, w) == (3, n_left + 1 + n_right)
        seen_left.add(n_left)
        seen_right.add(n_right)
    assert {63, 64, 65, 128} <= seen_left and {63, 64, 65, 128} <= seen_right
    win = cm.search(cc.CASES["finalise_reaches_column_0"])
    assert win.rect[1] == 0 and win.j > 0
    mask = cc.CASES["finalise_reaches_last_column"]
    win = cm.search(mask)
    assert win.rect[1] > 0 and win.rect[1] + win.rect[3] == mask.shape[1]
    mask = cc.CASES["finalise_reaches_both_ends"]
    assert cm.search(mask).rect[1::2] == (0, mask.shape[1])


# ------------------------------------------------------------------------------ heights scan
def test_heights_scan_cases():
    assert cc.SCAN_HEIGHTS == (1, 15, 16, 17, 31, 32, 33, 47) and cc.SCAN_W > 64
    for H in cc.SCAN_HEIGHTS:
        hs = (H + 15) // 16
        full = cm.heights(cc.CASES[f"scan_valid_throughout_{H}x{cc.SCAN_W}"])
        assert np.all(full == np.arange(1, H + 1)[:, None])
        off = cc.CASES[f"scan_last_row_invalid_{H}x{cc.SCAN_W}"]
        hgt = cm.heights(off)
        assert np.all(hgt[H - 1, ::3] == 0) and np.all(hgt[H - 1, 1::3] == H)
        assert H == 1 or np.all(hgt[H - 2] == H - 1)
        runs = cm.heights(cc.CASES[f"scan_runs_over_three_segments_{H}x{cc.SCAN_W}"])
        # some run starts in one segment and ends three segments further down, carried through
        # two whole segments in between
        ends = np.argwhere((runs > 0) & np.vstack((runs[1:] == 0, np.ones((1, cc.SCAN_W), bool))))
        spans = {(int(i) - int(runs[i, j]) + 1) // hs - int(i) // hs for i, j in ends}
        assert (-3 in spans) == (H > 3 * hs), (H, spans)      # (H = 1 has one segment)


# ---------------------------------------------------------------------------- values, random
def test_value_case_holds_only_0_2_and_255():
    mask = cc.CASES[cc.VALUES[0]]
    assert sorted(np.unique(mask).tolist()) == [0, 2, 255]
    assert cm.crop_rect(mask) == cm.crop_rect((mask != 0).astype(np.uint8))


def test_skylines_tie_often():
    assert len(cc.SKYLINES) == cc.N_SKYLINES == 200
    tied = plateaus = flipped = 0
    for s, name in enumerate(cc.SKYLINES):
        mask = cc.CASES[name]
        assert mask.shape[0] <= 8 and mask.shape[1] <= 400
        assert np.array_equal(mask, cc.skyline(s))                     # deterministic
        _, left, _, area = cm.candidates(mask)
        best = area == area.max()
        # the largest area at more than one (row, left) - distinct rectangles, not one rectangle
        # seen from several of its columns
        tied += len({(int(i), int(left[i, j])) for i, j in np.argwhere(best)}) > 1
        plateaus += s % 2
        flipped += bool(s & 2)
    print(f"{tied} of {cc.N_SKYLINES} skylines have several rectangles of the largest area")
    assert plateaus == flipped == 100
    assert tied >= 40                       # (the seeds are fixed: 45)
