"""CPU: the model of ``pano_overlap_stats``'s contract (tests/overlap_model.py) against the C oracle
and oracle/cv2_shim.py on every forged case of tests/overlap_cases.py, and the property each family
of cases claims, evaluated on the model alone - a case that lost its edge fails here.  Counts, masks
and samples by equality; the means to the accuracy of the oracle's float32 ``np.mean``."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_cases as oc  # noqa: E402
import overlap_model as om  # noqa: E402

MEAN_RTOL = 2e-6            # what test_overlap_stats_match_oracle grants np.mean's float32 sum


@functools.lru_cache(maxsize=None)
def _stats(name, k, rounding="even", split=True):
    case = oc.CASES[name]
    minv, i, j = case.pairs[k]
    return om.overlap(case.frames[i], case.frames[j], minv, case.bw0, case.hat_x, case.hat_y,
                      rounding, split)


def _pairs(names):
    return [(name, k) for name in names for k in range(len(oc.CASES[name].pairs))]


def _rgba(case, index):
    out = np.empty((case.h, case.w, 4), np.float32)
    out[..., :3] = om.LUT255[case.frames[index]]
    out[..., 3] = (case.hat_y[:, None] * case.hat_x[None, :]).astype(np.float32)
    return out


def _tiles(case):
    """(x0, y0, xe, ye) of every tile, last pixel inclusive."""
    return [(x0, y0, min(x0 + oc.TILE_W, case.w) - 1, min(y0 + oc.TILE_H, case.h) - 1)
            for y0 in range(0, case.h, oc.TILE_H) for x0 in range(0, case.w, oc.TILE_W)]


def _corners(minv, tile):
    """What the kernel's cull reads off a tile: the number of positive and of negative corner
    denominators, and the bounding box (lo_x, hi_x, lo_y, hi_y) of the corners' images, NaNs
    ignored as fmin / fmax ignore them."""
    x0, y0, xe, ye = tile
    cx, cy = np.array([x0, xe, x0, xe], float), np.array([y0, y0, ye, ye], float)
    with np.errstate(all="ignore"):
        den = minv[6] * cx + minv[7] * cy + minv[8]
        u = (minv[0] * cx + minv[1] * cy + minv[2]) / den
        v = (minv[3] * cx + minv[4] * cy + minv[5]) / den
    box = (np.fmin.reduce(u), np.fmax.reduce(u), np.fmin.reduce(v), np.fmax.reduce(v))
    return int((den > 0).sum()), int((den < 0).sum()), box


def _misses(box, case, slack=2.0):
    lo_x, hi_x, lo_y, hi_y = box
    return bool(hi_x < -slack or lo_x > case.w - 1 + slack or hi_y < -slack
                or lo_y > case.h - 1 + slack)


def _in_tile(mask, tile):
    x0, y0, xe, ye = tile
    return int(mask[y0:ye + 1, x0:xe + 1].sum())


# ------------------------------------------------------------------- the model and the oracle
def test_model_equals_the_oracle_on_every_case(oracle):
    lib = oracle.lib()
    worst = 0.0
    for name, case in oc.CASES.items():
        rgba = [_rgba(case, n) for n in range(len(case.frames))]
        for k, (minv, i, j) in enumerate(case.pairs):
            size, mean_i, mean_j = C.c_double(-1), C.c_float(-1), C.c_float(-1)
            m = np.ascontiguousarray(minv)
            lib.orc_overlap_stats(rgba[i].ctypes.data_as(C.c_void_p),
                                  rgba[j].ctypes.data_as(C.c_void_p), C.c_int(case.h),
                                  C.c_int(case.w), m.ctypes.data_as(C.c_void_p), C.c_int(case.bw0),
                                  C.byref(size), C.byref(mean_i), C.byref(mean_j))
            got = _stats(name, k)
            assert got.count == size.value == int(got.mask.sum()), (name, k)
            assert got.samples.shape == (got.count, 3) and got.samples.dtype == np.float32
            if got.count:
                means = np.array([got.sum_i, got.sum_j]) / (3.0 * got.count)
                want = np.array([mean_i.value, mean_j.value], np.float64)
                worst = max(worst, float(np.max(np.abs(means - want) / want)))
                np.testing.assert_allclose(means, want, rtol=MEAN_RTOL, atol=0, err_msg=name)
            else:
                assert got.sum_i == got.sum_j == 0.0 == mean_i.value == mean_j.value, (name, k)
    print(f"largest relative difference of a mean from the oracle's float32 mean: {worst:.2e}")


def test_model_equals_the_shim_bit_for_bit():
    """``cv2_shim.warpPerspective`` inverts its matrix itself: it is given invert3x3(minv), and the
    model the inverse of that, which is the case's own minv wherever the inversion is exact
    (the translations: every tie and cull-edge case)."""
    import cv2_shim
    n = exact = 0
    for name, case in oc.CASES.items():
        if case.hats != "engine" or case.bw0 != oc.warp_bw0(case.h, case.w):
            continue
        rgba = [_rgba(case, k) for k in range(len(case.frames))]
        for minv, i, j in case.pairs:
            hom = cv2_shim.invert3x3(minv.reshape(3, 3))
            back = cv2_shim.invert3x3(hom).ravel()
            if not (hom.any() and back.any() and np.isfinite(back).all()):
                continue                                   # singular
            want = cv2_shim.warpPerspective(rgba[j], hom, (case.w, case.h), cv2_shim.INTER_LINEAR,
                                            cv2_shim.BORDER_TRANSPARENT)
            got = om.overlap(case.frames[i], case.frames[j], back, case.bw0, case.hat_x, case.hat_y)
            assert np.array_equal(got.mask, want[..., 3] != 0), name
            assert got.samples.tobytes() == want[got.mask][:, :3].tobytes(), name
            n += 1
            exact += np.array_equal(back, minv)
            if name in oc.TIES:
                assert np.array_equal(back, minv), name
    print(f"{n} pairs compared with the shim, {exact} of them on the case's own minv")
    assert n >= 150 and exact >= 40


def test_cases_are_complete_and_small():
    names = (oc.SIZES + oc.TIES + oc.HORIZON + list(oc.ZERO_DEN) + oc.CULL + oc.MAGNIFY
             + list(oc.BLOCKWIDTH) + oc.BLOCKWIDTH_VARIANTS + oc.RANDOM)
    assert sorted(names) == sorted(oc.CASES)                # every case belongs to one family
    from pano360_amd import engine
    for name, case in oc.CASES.items():
        n = len(case.frames)
        assert case.frames.shape == (n, case.h, case.w, 3) and case.frames.dtype == np.uint8, name
        assert 2 <= n <= 4 and case.h <= 48 and case.w <= 640 and case.bw0 > 0, name
        assert len(np.unique(case.frames)) > min(200, case.frames.size // 2), name   # noise
        if case.hats == "engine":
            assert case.hat_x.tobytes() == engine.hat(case.w).tobytes(), name
            assert case.hat_y.tobytes() == engine.hat(case.h).tobytes(), name
        else:
            assert np.all(case.hat_x == 1) and np.all(case.hat_y == 1), name
        for minv, i, j in case.pairs:
            assert minv.shape == (9,) and minv.dtype == np.float64 and 0 <= i < n and 0 <= j < n
    assert len(oc.SIZES) == 2 * 36 and len(oc.RANDOM) == oc.N_RANDOM == 60
    for name in oc.SIZES + oc.RANDOM:
        case = oc.CASES[name]
        assert case.bw0 == min(1024 // min(16, case.h), case.w), name
    assert {oc.CASES[n].bw0 for n in oc.SIZES} == {2, 63, 64, 65, 68, 129, 130}
    assert sum(_stats(n, k).count > 0 for n, k in _pairs(oc.RANDOM)) >= 100


# -------------------------------------------------------------------------------------- ties
def test_every_tie_changes_under_round_half_away():
    assert len(_pairs(oc.TIES)) == 12
    for name, k in _pairs(oc.TIES):
        case = oc.CASES[name]
        big_x, big_y = om.fixed_point(case.pairs[k][0], case.h, case.w, case.bw0)
        tx, ty = case.pairs[k][0][[2, 5]] * 64
        assert tx % 2 == 1 and ty % 2 == 1                                   # odd multiples of 1/64
        away_x, away_y = om.fixed_point(case.pairs[k][0], case.h, case.w, case.bw0, "away")
        assert np.any(big_x != away_x) or np.any(big_y != away_y), (name, k)
        even, away = _stats(name, k), _stats(name, k, rounding="away")
        assert (even.count, even.sum_j) != (away.count, away.sum_j), (name, k)
        assert even.count > 900


# ----------------------------------------------------------------------------------- horizon
def test_horizon_cases_are_decided_by_the_sign_test():
    """A tile with counted pixels whose corner denominators do not share a sign; in the guarded
    cases the box of that tile's corner images misses frame j, so the sign test alone keeps it."""
    for name, k in _pairs(oc.HORIZON_GUARDED):
        case = oc.CASES[name]
        minv = case.pairs[k][0]
        den = om.denominators(minv, case.h, case.w, case.bw0)
        assert np.any(den < 0) and np.any(den > 0), name
        mask = _stats(name, k).mask
        guarded = 0
        for tile in _tiles(case):
            pos, neg, box = _corners(minv, tile)
            if pos != 4 and neg != 4 and _misses(box, case):
                guarded += _in_tile(mask, tile)
        assert guarded >= 20, (name, guarded)
    # through a corner: one corner denominator is exactly 0, the others of both signs
    case = oc.CASES["horizon_through_a_tile_corner_ones"]
    x, y = oc.HORIZON_CORNER_PIXEL
    tile = next(t for t in _tiles(case) if t[0] == x and t[3] == y)
    assert _corners(case.pairs[0][0], tile)[:2] == (1, 2)
    assert om.denominators(case.pairs[0][0], case.h, case.w, case.bw0)[y, x] == 0.0
    # through one tile only
    case = oc.CASES["horizon_oblique_through_one_tile_ones"]
    mixed = [t for t in _tiles(case) if 4 not in _corners(case.pairs[0][0], t)[:2]]
    assert mixed == [(0, 0, 63, 15)]


def test_negative_denominators_everywhere():
    for name in oc.HORIZON_NEGATIVE:
        case = oc.CASES[name]
        assert np.array_equal(case.pairs[0][0], -case.pairs[1][0])
        assert np.all(om.denominators(case.pairs[0][0], case.h, case.w, case.bw0) < 0), name
        neg, pos = _stats(name, 0), _stats(name, 1)
        assert neg.count == pos.count > 0 and np.array_equal(neg.mask, pos.mask)
        assert neg.samples.tobytes() == pos.samples.tobytes()
    case = oc.CASES["horizon_negative_everywhere_33x130_engine"]
    culled = [t for t in _tiles(case) if _corners(case.pairs[0][0], t)[1] == 4
              and _misses(_corners(case.pairs[0][0], t)[2], case)]
    assert len(culled) == 8 and len(_tiles(case)) == 9


# -------------------------------------------------------------------------- zero denominator
def test_zero_denominator_counts_through_tap_0_0_with_ones_only():
    assert len(oc.ZERO_DEN) == 6
    for name, pixels in oc.ZERO_DEN.items():
        case = oc.CASES[name]
        for k, (minv, i, j) in enumerate(case.pairs):
            den = om.denominators(minv, case.h, case.w, case.bw0)
            zero = np.argwhere(den == 0.0)
            if pixels is None:
                assert len(zero) == case.h * case.w and not minv.any()
            else:
                assert sorted((int(x), int(y)) for y, x in zero) == sorted(pixels), name
            sx, sy, fx, fy, inside = om.taps(minv, case.h, case.w, case.bw0)
            got = _stats(name, k)
            order = np.cumsum(got.mask.ravel()) - 1             # index into samples, row-major
            for y, x in zero:
                assert (sx[y, x], sy[y, x], fx[y, x], fy[y, x]) == (0, 0, 0, 0) and inside[y, x]
                assert bool(got.mask[y, x]) == (case.hats == "ones"), (name, x, y)
                if got.mask[y, x]:
                    sample = got.samples[order[y * case.w + x]]
                    assert np.array_equal(sample, om.LUT255[case.frames[j][0, 0]]), (name, x, y)
        assert case.hat_x[0] * case.hat_y[0] == (1.0 if case.hats == "ones" else 0.0)


# -------------------------------------------------------------------------------- cull edges
def test_cull_edges_step_across_the_rounding_boundary():
    assert oc.CULL_STEPS == tuple(range(-4, 5))
    for name, (col, row) in {**oc.CULL_LOW, **oc.CULL_HIGH}.items():
        case = oc.CASES[name]
        tile = next(t for t in _tiles(case) if t[:2] == (col * oc.TILE_W, row * oc.TILE_H))
        assert len(case.pairs) == len(oc.CULL_STEPS) and case.hats == "ones"
        for k, step in enumerate(oc.CULL_STEPS):
            pos, neg, (lo_x, hi_x, lo_y, hi_y) = _corners(case.pairs[k][0], tile)
            assert pos == 4
            counted = _in_tile(_stats(name, k).mask, tile)
            if name in oc.CULL_LOW:
                # the tile's largest coordinate is step / 128: tap 0 from -1/64 upwards
                assert (hi_x if name.endswith("x") else hi_y) == step / 128
                assert (counted > 0) == (step / 128 >= -1 / 64), (name, step)
                assert counted in (0, oc.TILE_H if name.endswith("x") else oc.TILE_W)
                # -1/64 and -1/128: counted pixels in a tile whose box lies wholly below 0
                assert not _misses((lo_x, hi_x, lo_y, hi_y), case)
                assert _misses((lo_x, hi_x, lo_y, hi_y), case, slack=0.0) == (step < 0)
            else:
                edge = (case.w if name.endswith("x") else case.h) - 1
                assert (lo_x if name.endswith("x") else lo_y) == edge + step / 128
                assert (counted > 0) == (step / 128 < -1 / 64), (name, step)
                assert not _misses((lo_x, hi_x, lo_y, hi_y), case)


def test_culled_footprints():
    case = oc.CASES[oc.CULL_ALL]
    for k, (minv, i, j) in enumerate(case.pairs):
        assert _stats(oc.CULL_ALL, k).count == 0
        assert all(_corners(minv, t)[0] == 4 and _misses(_corners(minv, t)[2], case)
                   for t in _tiles(case))
    case = oc.CASES[oc.CULL_ALL_BUT_ONE]
    minv = case.pairs[0][0]
    kept = [t for t in _tiles(case) if not _misses(_corners(minv, t)[2], case)]
    assert kept == [(64, 16, 127, 31)] and len(_tiles(case)) == 9
    got = _stats(oc.CULL_ALL_BUT_ONE, 0)
    assert got.count == _in_tile(got.mask, kept[0]) > 200


# ----------------------------------------------------------------------------- magnification
def test_magnifications_clamp_and_saturate():
    for tag, clamps in (("1e6", True), ("1e12", True), ("65537", False)):
        case = oc.CASES[f"magnify_{tag}_ones"]
        big_x, _ = om.fixed_point(case.pairs[0][0], case.h, case.w, case.bw0)
        sx = om.taps(case.pairs[0][0], case.h, case.w, case.bw0)[0]
        assert (big_x.max() == 2 ** 31 - 1) == clamps
        assert (big_x >> 5).max() > 32767 == sx.max()
        assert _stats(f"magnify_{tag}_ones", 0).count == 1               # pixel (0, 0) alone
        assert _stats(f"magnify_{tag}_engine", 0).count == 0
    # cut to 16 bits instead of saturated, these taps would lie inside the frame
    case = oc.CASES["magnify_65537_ones"]
    wrapped = ((om.fixed_point(case.pairs[0][0], case.h, case.w, case.bw0)[0] >> 5) + 32768) % 65536
    assert np.array_equal(wrapped[0] - 32768, np.arange(case.w))
    case = oc.CASES["magnify_shift_by_65536_ones"]
    for k in (0, 1):
        big = om.fixed_point(case.pairs[k][0], case.h, case.w, case.bw0)[k] >> 5
        assert np.all((big + 32768) % 65536 - 32768 == np.arange(case.h if k else case.w)[
            (slice(None), None) if k else (None, slice(None))])
        assert _stats("magnify_shift_by_65536_ones", k).count == 0
    for hats in ("ones", "engine"):
        name = f"minify_into_one_texel_{hats}"
        case = oc.CASES[name]
        sx, sy = om.taps(case.pairs[0][0], case.h, case.w, case.bw0)[:2]
        assert np.all(sx == oc.MINIFY_TEXEL[0]) and np.all(sy == oc.MINIFY_TEXEL[1])
        assert _stats(name, 0).count == case.h * case.w
    case = oc.CASES["magnify_3_ones"]
    assert _stats("magnify_one_third_ones", 0).count == case.h * case.w
    assert 0 < _stats("magnify_3_ones", 0).count < case.h * case.w // 8


# ------------------------------------------------------------------------------- block width
def test_every_block_width_case_changes_without_the_split():
    assert len(oc.BLOCKWIDTH) == len(oc.BLOCKWIDTH_SHAPES) == 4
    assert len(oc.BLOCKWIDTH_VARIANTS) == 8
    for name, (x, y) in oc.BLOCKWIDTH.items():
        case = oc.CASES[name]
        assert 9 <= case.h <= 15 and 200 <= case.w <= 640 and case.bw0 == 1024 // case.h != 64
        minv = case.pairs[0][0]
        assert minv[6] != 0 and minv[7] != 0 and np.frexp(minv[0])[0] != 0.5
        split = om.fixed_point(minv, case.h, case.w, case.bw0)
        whole = om.fixed_point(minv, case.h, case.w, case.bw0, split=False)
        assert split[0][y, x] != whole[0][y, x] and x >= case.bw0 and x % case.bw0, name
        one_block = om.fixed_point(minv, case.h, case.w, case.w)
        assert split[0][y, x] != one_block[0][y, x], name
        with_split, without = _stats(name, 0), _stats(name, 0, split=False)
        assert with_split.mask[y, x] and without.mask[y, x], name
        assert with_split.samples.tobytes() != without.samples.tobytes(), name
        assert with_split.sum_j != without.sum_j, name
        for variant in (name + "_bw64", name + "_bw_w"):
            other = oc.CASES[variant]
            assert variant in oc.BLOCKWIDTH_VARIANTS and np.array_equal(other.pairs[0][0], minv)
            assert other.bw0 == (64 if variant.endswith("64") else case.w)


# -------------------------------------------------------------------------- the pair table
def test_overlap_pairs_equal_the_oracle_bit_for_bit(oracle):
    from pano360_amd import engine, synth
    n, w, h = 6, 130, 17
    rots, intrs = synth.make_cameras(n, w, h, sweep_deg=150.0, jitter=0.02, seed=3)
    table = engine.overlap_pairs(rots, intrs, w, h)
    want = []
    for i in range(n):
        for j in range(i + 1, n):
            hom, behind = oracle.pair_homography(rots[i], intrs[i], rots[j], intrs[j], w, h)
            if not behind:
                want.append((oracle.invert3x3(hom).ravel(), i, j))
    assert 3 <= len(want) == len(table) < n * (n - 1) // 2
    for rec, (minv, i, j) in zip(table, want):
        assert (int(rec["i"]), int(rec["j"])) == (i, j)
        assert rec["minv"].tobytes() == minv.tobytes(), (i, j)
