"""The MSOP model (tests/msop_model.py) against the reference's recorded results
(tests/golden/msop_*.npz, written by tools/gen_msop_golden.py), on the CPU.

The model is the specification of csrc/msop.hip; tests/test_gpu_msop.py holds the kernels to
it.  Here it is held to the reference: the per-level cut lists, the ``ssc`` selections and the
point tuples are equal (theta as float32 bits).  Descriptors: the reference inverts its float32
matrix through LAPACK where the model uses the closed form of the map, which moves some sample
coordinates across a 1/32 rounding boundary - at most 5 % of a fixture's patches may differ at
all, and then by no more than twice the worst difference the generator measured for that
fixture (a rounding flip of one tap, not a different patch).
"""
import functools
import math
import os

import numpy as np
import pytest

import msop_model as mm
from conftest import GOLDEN

FIXTURES = ("noise", "odd", "flat")


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(GOLDEN, f"msop_{name}.npz")) as g:
        return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def model(name):
    """The model's stages, fed the reference's own angles (so the patches are comparable)."""
    g = golden(name)
    max_feat = tuple(int(v) for v in g["max_feat"])
    own = mm.detect(g["img"], max_feat, want_stages=True)
    theta, start, per_level = g["points"][:, 2].astype(np.float32), 0, []
    for lvl in range(len(max_feat)):
        n = int(np.sum(g["points"][:, 3] == 2 ** lvl))
        per_level.append(theta[start:start + n])
        start += n
    fed = mm.detect(g["img"], max_feat, thetas_in=per_level)
    return own, fed


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_the_seeded_input(name):
    g = golden(name)
    assert np.array_equal(g["img"], mm.fixture_image(name))
    assert g["img"].dtype == np.uint8 and g["points"].dtype == np.float64
    n_levels = len(g["max_feat"])
    assert all(len(g[f"ssc_out_{lvl}"]) >= 4 for lvl in range(n_levels))
    assert sum(len(g[f"ssc_out_{lvl}"]) for lvl in range(n_levels)) == len(g["points"])


@pytest.mark.parametrize("name", FIXTURES)
def test_cut_lists_and_selections_equal_the_reference(name):
    g = golden(name)
    stages = model(name)[0][2]
    for lvl, st in enumerate(stages):
        assert np.array_equal(st["cut"], g[f"ssc_in_{lvl}"]), f"level {lvl}: the cut differs"
        assert np.array_equal(st["cut"][st["sel"]], g[f"ssc_out_{lvl}"]), \
            f"level {lvl}: the ssc selection differs"


def test_the_cut_is_exercised_and_has_ties():
    """noise and flat cut level 0 down to 20 maxf; flat's saturated rectangles are plateaus of
    response exactly 0, candidates as a whole, and responses repeat among the candidates."""
    for name in ("noise", "flat"):
        g = golden(name)
        assert len(g["ssc_in_0"]) == 20 * int(g["max_feat"][0])
    hrs = model("flat")[0][2][0]["hrs"]
    assert (hrs[25:55, 35:85] == 0).all() and (hrs[105:145, 145:215] == 0).all()
    pos = mm.candidates(hrs)
    assert np.isin(np.ravel_multi_index((40, 60), hrs.shape), pos)
    values = hrs.reshape(-1)[pos]
    assert len(np.unique(values)) < len(values)


@pytest.mark.parametrize("lvl", (1, 2))
def test_ties_straddle_the_cut_of_flat(lvl):
    """What the flat fixture is for: at levels 1 and 2 the weakest response kept by the cut is
    shared with a candidate the cut drops, so the order of equal responses decides the list; and
    responses repeat inside the cut as well."""
    g = golden("flat")
    hrs = model("flat")[0][2][lvl]["hrs"]
    keep = 20 * int(g["max_feat"][lvl])
    values = np.sort(hrs.reshape(-1)[mm.candidates(hrs)] + np.float32(0))
    assert len(values) > keep
    assert values[-keep - 1] == values[-keep]
    assert len(np.unique(values[-keep:])) < keep


@pytest.mark.parametrize("name", FIXTURES)
def test_points_equal_the_reference(name):
    g = golden(name)
    points = model(name)[0][0]
    assert points.shape == g["points"].shape
    assert np.array_equal(points[:, [0, 1, 3]], g["points"][:, [0, 1, 3]])
    assert np.array_equal(points[:, 2].astype(np.float32).view(np.uint32),
                          g["points"][:, 2].astype(np.float32).view(np.uint32))
    assert np.array_equal(points[:, 2], g["points"][:, 2])      # float64 of a float32


@pytest.mark.parametrize("name", FIXTURES)
def test_descriptors_against_the_reference(name):
    g = golden(name)
    descs = model(name)[1][1]
    assert descs.shape == g["descs"].shape and descs.dtype == np.float32
    diff = np.abs(descs.astype(np.float64) - g["descs"].astype(np.float64)).max(axis=1)
    n_diff, worst = int(np.count_nonzero(diff)), float(diff.max())
    print(f"{name}: {n_diff} of {len(descs)} patches differ, worst {worst:.4g} "
          f"(recorded worst {float(g['desc_worst']):.4g})")
    assert n_diff <= 0.05 * len(descs)
    assert worst <= 2 * float(g["desc_worst"])


def test_descriptors_are_normalised():
    """A normalised value is at most sqrt(64) = 8 in magnitude and carries the float32 roundings
    of the mean, the subtraction and the division: a few times 8 x 2^-24 = 5e-7 each, and the
    mean of 64 of them no more - 1e-5 bounds both."""
    descs = model("noise")[0][1].astype(np.float64)
    assert np.abs(descs.mean(axis=1)).max() < 1e-5
    assert np.abs(descs.std(axis=1) - 1).max() < 1e-5


def test_patch_closed_form_equals_the_general_warp_where_the_matrix_is_exact():
    """For theta = 0 the reference's matrix and its inverse are exact in float32, so the general
    warp (the matrix inverted again in double) and the closed form agree to the bit."""
    blurred = mm.gradient_planes(mm.gray_u8(mm.fixture_image("odd")))[2]
    theta = np.float32(0.0)
    for r, c in ((40, 50), (0, 0), (156, 202), (3, 200)):
        rmat = np.linalg.inv(mm.rot_mat(theta, (r, c)))
        rmat[:2, 2] += mm.DSIZE / 2
        tile = mm.warp_perspective(blurred, rmat, (mm.DSIZE, mm.DSIZE))
        assert np.array_equal(tile, mm.patches(blurred, [theta], [r], [c])[0])
        assert tile.any()
    # away from the image the constant border gives zeros
    assert not mm.patches(blurred, [np.float32(0.3)], [-40], [-40]).any()


# ------------------------------------------------------------------ ssc
def ssc_literal(keypoints, im_size, n_points, tol=0.1):
    """features.py:27-99 restated without a coverage grid: a point is taken when no point taken
    before it lies within ``floor(width / cgr)`` cells of its own cell in both directions (the
    clipped box of a taken point covers exactly those cells of the grid)."""
    cols, rows = im_size                         # the reference's swap: im_size is (H, W)
    # the search range: the roots of (n - 1) w^2 + 2 s w + 4 (n + cols - rows cols) = 0
    n, s = n_points, rows + cols + 2 * n_points
    under_root = s * s - 4 * (n - 1) * (n + cols - rows * cols)
    roots = [(-s + sign * math.sqrt(under_root)) / (n - 1) for sign in (1, -1)]
    high = max(round(w) for w in roots)          # Python's round: half to even
    low = math.floor(math.sqrt(len(keypoints) / n))
    k_min, k_max = round(n - n * tol), round(n + n * tol)
    prev_width = -1
    result, exit_by = [], None
    while True:
        width = low + (high - low) / 2
        if width == prev_width:
            exit_by = "same width"
            break
        if low > high:
            exit_by = "low > high"
            break
        cgr = width / 2
        reach = math.floor(width / cgr)
        taken, result = [], []
        for i, kpt in enumerate(keypoints):
            row, col = int(math.floor(kpt[1] / cgr)), int(math.floor(kpt[0] / cgr))
            if all(abs(row - r) > reach or abs(col - c) > reach for r, c in taken):
                taken.append((row, col))
                result.append(i)
        if k_min <= len(result) <= k_max:
            exit_by = "found"
            break
        if len(result) < k_min:
            high = width - 1
        else:
            low = width + 1
        prev_width = width
    return result, exit_by, cgr


def random_points(h, w, n, seed):
    flat = np.random.default_rng(seed).choice(h * w, n, replace=False)
    return np.stack([flat // w, flat % w], axis=1)


# (h, w, points, n_points, seed, how the search ends)
SSC_CASES = ((192, 256, 3000, 200, 5, "found"),
             (192, 256, 40, 50, 5, "low > high"),        # fewer points than asked: cgr < 1
             (64, 80, 296, 56, 4, "low > high"),
             (64, 80, 33, 42, 23, "low > high"),         # a grid past the on-chip bitmap
             (192, 256, 300, 40, 5, "found"),
             (48, 40, 500, 9, 2, None))


@pytest.mark.parametrize("h,w,n,n_points,seed,ends", SSC_CASES)
def test_ssc_model_equals_the_literal_restatement(h, w, n, n_points, seed, ends):
    if (h, w) == (64, 80):
        rng = np.random.default_rng(seed)        # the draw the case was found with
        assert (int(rng.integers(20, 400)), int(rng.integers(3, 60))) == (n, n_points)
        flat = rng.choice(h * w, n, replace=False)
        pts = np.stack([flat // w, flat % w], axis=1)
    else:
        pts = random_points(h, w, n, seed)
    want, exit_by, cgr = ssc_literal(pts, (h, w), n_points)
    assert mm.ssc_indices(pts, (h, w), n_points) == want
    assert [tuple(p) for p in mm.ssc(pts, (h, w), n_points)] == [tuple(pts[i]) for i in want]
    if ends is not None:
        assert exit_by == ends
    if n < n_points:
        assert cgr < 1 and len(want) == n


def test_ssc_search_ends_as_the_cases_say():
    """The model's own search control ends the named cases the way the table says, after at least
    two probes."""
    for h, w, n, n_points, seed, ends in SSC_CASES[:4]:
        if (h, w) == (64, 80):
            rng = np.random.default_rng(seed)
            rng.integers(20, 400), rng.integers(3, 60)
            flat = rng.choice(h * w, n, replace=False)
            pts = np.stack([flat // w, flat % w], axis=1)
        else:
            pts = random_points(h, w, n, seed)
        search, probes = mm.SscSearch(len(pts), (h, w), n_points), 0
        while search.next_width() is not None:
            search.report(len(mm.ssc_probe(pts, *search.grid())))
            probes += 1
        assert probes >= 2
        assert search.complete if ends == "found" else search.low > search.high


def test_value_errors():
    pts = random_points(32, 32, 50, 1)
    with pytest.raises(ValueError):
        mm.ssc_indices(pts, (32, 32), 1)
    # a constant 5 x 5 frame: 25 candidates, and for two points the search range is empty
    # (low 3 > high 2) before any probe - the reference stacks an empty list there
    with pytest.raises(ValueError):
        mm.detect(np.full((5, 5, 3), 90, np.uint8), (2,))
