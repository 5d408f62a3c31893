"""CPU: the forged Poisson cases of tests/poisson_cases.py are what the GPU test takes them for.
Everything here is tests/poisson_model.py solved by SciPy's direct solver: the two classes, the
places the masks reach between them (computed from the masks), and what the clip case clips."""
import numpy as np
import pytest

import poisson_cases as pc
import poisson_model as pm

WAVE = 128                      # elements of a wave's pass in csrc/poisson.hip
TILE = 2048                     # elements of a block

GENERIC = sorted(n for n, c in pc.CASES.items() if c.cls == "generic")
INTEGRAL = sorted(n for n, c in pc.CASES.items() if c.cls == "integral")


def test_the_table_holds_what_the_tests_name():
    assert len(pc.CASES) == len(GENERIC) + len(INTEGRAL) == 45
    for name, case in pc.CASES.items():
        H, W = case.mask.shape
        assert case.src.shape == case.tgt.shape == (H, W, case.src.shape[2]), name
        assert case.src.dtype == case.tgt.dtype == np.uint8 and case.mask.dtype == bool, name
        assert 1 <= case.src.shape[2] <= 4 and W >= 2 and H * W <= 67 * 131, name
        assert case.mask.any(), name
        assert not any(a.flags.writeable for a in case[:3]), name
    for i in pc.SINGLES:
        m = pc.CASES[f"single_{i}"].mask.reshape(-1)
        assert m.sum() == 1 and m[i]
    import test_gpu_poisson as fixtures_test
    assert pc.GUARD == fixtures_test.GUARD == 1e-4
    assert pc.LEFT_OUT == fixtures_test.LEFT_OUT == 0.002


@pytest.mark.parametrize("name", GENERIC)
def test_generic_case_is_within_the_cap(name):
    """At most LEFT_OUT of the mask per channel within GUARD of an integer; under 500 mask
    pixels that is none."""
    share = pc.near_integer_share(name)
    assert (share <= pc.LEFT_OUT).all(), share
    if pc.CASES[name].mask.sum() < 500:
        assert (share == 0).all(), share


@pytest.mark.parametrize("name", INTEGRAL)
def test_integral_case_needs_its_waiver(name):
    share = pc.near_integer_share(name)
    assert (share > pc.LEFT_OUT).any(), share
    if name == "same_channel":
        assert (share[list(pc.SAME_GENERIC)] <= pc.LEFT_OUT).all() and share[1] == 1.0, share


def flat_neighbours(mask):
    """bool[4][N]: the flat neighbour i-1, i+1, i-W, i+W exists and is a mask pixel."""
    H, W = mask.shape
    m = mask.reshape(-1)
    N = m.size
    i = np.arange(N)
    out = []
    for off in (-1, 1, -W, W):
        n = i + off
        ok = (n >= 0) & (n < N)
        out.append(ok & m[np.clip(n, 0, N - 1)])
    return np.array(out)


def group_is_empty(mask, n, size):
    """Per flat index in n (clipped into the image): its aligned group of ``size`` elements
    holds no mask pixel, so the wave (128) or block (2048) that owns it skips the pass."""
    m = mask.reshape(-1)
    pad = np.zeros(-(-m.size // size) * size, bool)
    pad[:m.size] = m
    empty = ~pad.reshape(-1, size).any(axis=1)
    return empty[np.clip(n, 0, m.size - 1) // size]


def places(mask):
    H, W = mask.shape
    m = mask.reshape(-1)
    N = m.size
    i = np.arange(N)
    x = i % W
    nb = flat_neighbours(mask)
    alone = m & ~nb.any(axis=0)
    left_skipped = (i >= 1) & group_is_empty(mask, i - 1, WAVE)
    right_skipped = (i + 1 < N) & group_is_empty(mask, i + 1, WAVE)
    up_skipped = (i >= W) & group_is_empty(mask, i - W, WAVE)
    down_skipped = (i + W < N) & group_is_empty(mask, i + W, WAVE)
    return {
        "w == 2": W == 2,
        "w == 3": W == 3,
        "h == 1": H == 1,
        "full mask": m.all(),
        "full mask, odd h w": m.all() and N % 2 == 1,
        "x == 0": mask[:, 0].any(),
        "x == w-2": mask[:, -2].any(),
        "x == w-1": mask[:, -1].any(),
        "x == w-2 without x == w-1": (mask[:, -2] & ~mask[:, -1]).any(),
        "x == w-1 without x == w-2": (mask[:, -1] & ~mask[:, -2]).any(),
        "x == w-1 whose i+1 is a mask pixel": (m & (x == W - 1) & nb[1]).any(),
        "x == 0 whose i-1 is a mask pixel": (m & (x == 0) & nb[0]).any(),
        "x == 0 on an odd flat index": (m & (x == 0) & (i % 2 == 1)).any(),
        "x == 0 on an even flat index": (m & (x == 0) & (i % 2 == 0) & (i > 0)).any(),
        "first pixel": m[0],
        "last pixel": m[-1],
        "first row": mask[0].any(),
        "last row": mask[-1].any(),
        "alone on an even flat index": (alone & (i % 2 == 0)).any(),
        "alone on an odd flat index": (alone & (i % 2 == 1)).any(),
        "first of a wave, i-1 in a skipped wave": (m & (i % WAVE == 0) & left_skipped).any(),
        "last of a wave, i+1 in a skipped wave": (m & (i % WAVE == WAVE - 1)
                                                    & right_skipped).any(),
        "first of a block, i-1 in a skipped block": (
            m & (i % TILE == 0) & (i >= 1) & group_is_empty(mask, i - 1, TILE)).any(),
        "last of a block, i+1 in a skipped block": (
            m & (i % TILE == TILE - 1) & (i + 1 < N) & group_is_empty(mask, i + 1, TILE)).any(),
        "i-w in a skipped wave": (m & up_skipped).any(),
        "i+w in a skipped wave": (m & down_skipped).any(),
        "i-w in another block, skipped": (m & (i >= W) & ((i - W) // TILE != i // TILE)
                                          & up_skipped).any(),
        "i+w in another block, skipped": (m & (i + W < N) & ((i + W) // TILE != i // TILE)
                                          & down_skipped).any(),
        "mask pixels on both sides of a wave border": (m & (i % WAVE == WAVE - 1) & nb[1]).any(),
        "mask pixels on both sides of a block border": (m & (i % TILE == TILE - 1) & nb[1]).any(),
        "a mask pixel in a partial last block": N % TILE != 0 and m[N // TILE * TILE:].any(),
        "odd h w, last pixel masked": N % 2 == 1 and m[-1],
        "a wave without a mask pixel between two with": bool(
            np.diff(np.flatnonzero(np.pad(m, (0, -m.size % WAVE)).reshape(-1, WAVE).any(1)))
            .max(initial=0) > 1),
    }


def test_masks_reach_every_special_place():
    seen = {}
    for name, case in pc.CASES.items():
        for place, hit in places(case.mask).items():
            seen.setdefault(place, [])
            if hit:
                seen[place].append(name)
    missing = [place for place, names in seen.items() if not names]
    assert not missing, missing
    # the cases built for a place reach it
    assert "wrap" in seen["x == w-1 whose i+1 is a mask pixel"]
    assert "pair_over_row_end" in seen["x == w-1 whose i+1 is a mask pixel"]
    assert "blobs" in seen["mask pixels on both sides of a block border"]
    assert "single_2048" in seen["first of a block, i-1 in a skipped block"]
    assert "single_2047" in seen["last of a block, i+1 in a skipped block"]
    assert "full_45x91" in seen["odd h w, last pixel masked"]
    assert {"rows_7x2", "col1_7x2", "col0_7x2", "full_1x2", "full_2x2", "full_7x2"} \
        <= set(seen["w == 2"])


def test_blobs_cover_the_named_flat_indices():
    m = pc.CASES["blobs"].mask.reshape(-1)
    for i in (127, 128, 2047, 2048, 4095, 4096, 6143, 6144):
        assert m[i], i


def test_isolated_pixels_have_no_mask_neighbour():
    for name in ("isolated", "odd_flat", "even_flat", "one_pixel"):
        mask = pc.CASES[name].mask
        assert not (mask.reshape(-1) & flat_neighbours(mask).any(axis=0)).any(), name
    assert pc.CASES["isolated"].mask.sum() == 352


def test_isolated_solutions_are_quarters_and_every_channel_moves():
    """A = 4 I on an isolated mask: x = k / 4.  Every channel of the one-pixel case has r0 != 0,
    so it takes its one exact step."""
    for name in ("isolated", "one_pixel"):
        case = pc.CASES[name]
        sol, _ = pc.solved(name)
        inside = sol[:, case.mask]
        assert np.abs(inside * 4 - np.rint(inside * 4)).max() <= 1e-9, name
        moved = np.abs(inside - case.tgt.transpose(2, 0, 1)[:, case.mask]) >= 0.25
        assert moved.any(axis=1).all(), name
        if name == "one_pixel":
            assert moved.all()


def test_clip_case_clips_both_ways_and_next_to_the_bounds():
    case = pc.CASES["clip"]
    sol, image = pc.solved("clip")
    v = sol[:, case.mask]
    assert v.min() < -100 and v.max() > 355
    assert ((v > 0) & (v < 255)).any()
    # a truncation that forgot the clip would wrap these: (int)-0.5 is 0 but (uint8)255.5 is not
    assert ((v > -1) & (v < 0)).any() and ((v > 255) & (v < 256)).any()
    inside = image[case.mask]
    assert (inside == 0).any() and (inside == 255).any()


def test_converged_and_zero_channels_start_at_the_solution():
    """Channel 1 of same_channel and all of zero: b - A x0 = 0 exactly, in integers; and the
    zero case has b = 0."""
    for name, channels in (("same_channel", (1,)), ("zero", (0, 1, 2))):
        case = pc.CASES[name]
        for c in channels:
            b = pm.rhs(case.src[..., c], case.tgt[..., c], case.mask)
            r0 = b - pm.apply_A(case.tgt[..., c].astype(np.float64).reshape(-1), case.mask)
            assert not r0.any(), (name, c)
            if name == "zero":
                assert not b.any()
    case = pc.CASES["same_channel"]
    for c in pc.SAME_GENERIC:
        b = pm.rhs(case.src[..., c], case.tgt[..., c], case.mask)
        assert (b - pm.apply_A(case.tgt[..., c].astype(np.float64).reshape(-1), case.mask)).any()


def test_reference_solves_its_own_system():
    """The direct solve's residual on every case: the reference the GPU test compares with is
    good to far below GUARD."""
    for name, case in pc.CASES.items():
        sol, _ = pc.solved(name)
        for c in range(sol.shape[0]):
            b = pm.rhs(case.src[..., c], case.tgt[..., c], case.mask)
            r = b - pm.apply_A(sol[c].reshape(-1), case.mask)
            assert np.abs(r).max() <= 1e-9, (name, c, np.abs(r).max())
            assert np.abs(sol[c][~case.mask] - case.tgt[..., c][~case.mask]).max(initial=0) <= 1e-9
