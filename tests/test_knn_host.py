"""CPU: the NumPy model of ``pano_knn2`` (tests/knn_model.py) against exact arithmetic, and the
conditions that the cases of tests/test_gpu_knn.py depend on, evaluated on the model alone."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_model as km  # noqa: E402


def _nearest_f32(x):
    """The float32 nearest to the Fraction x, ties to the even mantissa."""
    r = np.float32(float(x))
    near = [np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf))]
    err = [abs(Fraction(float(c)) - x) for c in near]
    best = min(err)
    tied = [c for c, e in zip(near, err) if e == best]
    if len(tied) == 2:
        tied = [c for c in tied if not (c.view(np.uint32) & 1)]
    assert len(tied) == 1
    return tied[0]


def _fma_samples():
    rng = np.random.default_rng(21)
    n = 1000

    def mant(k):
        return (1.0 + rng.random(k)).astype(np.float32) * rng.choice((-1.0, 1.0), k).astype(np.float32)

    parts = []
    for shift in (0, 1, 12, 23, 24, 25, 30, 60, -1, -12, -24, -25, -40):   # acc / df^2 ~ 2^shift
        a = mant(n)
        parts.append((a, a if shift % 2 else mant(n), mant(n) * np.float32(2.0 ** shift)))
    a, b = mant(n), mant(n)
    parts.append((a, b, (-(a * b)).astype(np.float32)))            # cancellation: c ~ -ab
    parts.append((mant(n) * np.float32(1e-20), mant(n) * np.float32(1e-20), mant(n) * np.float32(1e-40)))
    # the float64 sum lands exactly on a float32 midpoint and the lost part decides:
    # 2^-24 (1 + 2^-11)(1 - 2^-11 + 2^-22) = 2^-24 + 2^-57, 2^-24 (1 + 2^-20)(1 - 2^-20) = 2^-24 - 2^-64
    c = np.array([1.0, 1.0 + 2.0 ** -23, 1.5, 1.5 + 2.0 ** -23, -1.0, -1.0 - 2.0 ** -23], np.float32)
    up = (np.float32(2.0 ** -24 * (1 + 2.0 ** -11)), np.float32(1 - 2.0 ** -11 + 2.0 ** -22))
    down = (np.float32(2.0 ** -24 * (1 + 2.0 ** -20)), np.float32(1 - 2.0 ** -20))
    for x, y in (up, down, (-up[0], up[1]), (-down[0], down[1])):
        parts.append((np.full(6, x), np.full(6, y), c))
    parts.append((np.full(6, np.float32(2.0 ** -24)), np.ones(6, np.float32), c))     # a true tie
    return tuple(np.concatenate([p[k] for p in parts]).astype(np.float32) for k in range(3))


def test_fma_rounds_once():
    """``fma32`` against Fraction arithmetic rounded once to float32: accumulators much larger
    and much smaller than the product, cancellation, the denormal range, and sums that sit on a
    float32 midpoint in float64 (where casting the float64 sum gives the other neighbour)."""
    a, b, c = _fma_samples()
    got = km.fma32(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    want = np.array([_nearest_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
                     for x, y, z in zip(a, b, c)], np.float32)
    print(f"{len(a)} samples, {int((naive != want).sum())} where rounding twice is wrong")
    assert (naive != want).any()                     # the samples include what the helper is for
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_wave_sum_is_the_butterfly():
    """Lane 0 of the full butterfly (every lane adds its partner l ^ 32, ^ 16, ... ^ 1)."""
    rng = np.random.default_rng(22)
    v = (rng.standard_normal((50, 64)) * 10.0 ** rng.integers(-3, 4, (50, 64))).astype(np.float32)
    full = v.copy()
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        full = full + full[:, lanes ^ o]
    assert np.array_equal(km.wave_sum32(v), full[:, 0])
    assert not np.array_equal(km.wave_sum32(v), v.sum(1, dtype=np.float32))    # the order matters


def test_integer_rows_are_exact():
    """Integer-valued rows: every step is exact (128 * 255^2 and 128 * 254^2 < 2^24)."""
    for gen in (km.uniform_int, km.signed_int):
        for d in (128, 64):
            q, t = gen(60, 90, d, 23)
            ref = ((q[:, None, :].astype(np.int64) - t[None].astype(np.int64)) ** 2).sum(-1)
            d2 = km.exact_d2(q, t)
            assert d2.dtype == np.float32 and np.array_equal(d2.astype(np.int64), ref)


def test_float_rows_are_within_rounding():
    """A sanity check of the derived order against a worst-case bound: a positive term passes at
    most ten roundings (the difference counts twice in its square, two FMAs, six additions of the
    tree), 10 * 2^-24 of the float64 sum; random rows stay well inside the 9 * 2^-24 = 5.4e-7
    asserted here (1.8e-7)."""
    worst = 0.0
    for d in (128, 100, 64, 5):
        q, t = km.uniform_float(60, 90, d, 24)
        ref = ((q[:, None, :].astype(np.float64) - t[None]) ** 2).sum(-1)
        worst = max(worst, float(np.max(np.abs(km.exact_d2(q, t) - ref) / ref)))
    print(f"largest relative deviation from the float64 sum: {worst:.2e}")
    assert worst <= 9 * 2.0 ** -24


def test_knn2_orders_ties_by_index():
    q = np.zeros((1, 4), np.float32)
    t = np.array([[2, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [3, 0, 0, 0]], np.float32)
    idx, dist = km.knn2(q, t)
    assert idx.dtype == np.int32 and idx.tolist() == [[1, 2]] and dist.tolist() == [[1.0, 1.0]]


def test_sift_like_rows_tie_by_themselves():
    q, t = km.sift_like()
    assert q.shape == (700, 128) and t.shape == (1333, 128)
    assert np.array_equal(q, np.round(q)) and q.min() >= 0 and q.max() <= 255
    s = km.sorted_d2(km.exact_d2(q, t), 3)
    first, second = int((s[:, 0] == s[:, 1]).sum()), int((s[:, 1] == s[:, 2]).sum())
    print(f"seed {km.SIFT_SEED}: {first} queries tie first / second, {second} second / third")
    assert first >= 5 and second >= 15


def test_planted_groups():
    """Groups of 2, 3, 5 and 6 equal rows, inside one tile on both halves of the wave and across
    tiles; queries equal to a row; the model answers with the two lowest rows of the group."""
    q, t, group = km.planted()
    assert sorted(len(g) for g in km.PLANTED_GROUPS) == [2, 3, 5, 5, 6, 6]
    same_tile_both_halves = 0
    for rows in km.PLANTED_GROUPS:
        assert all(np.array_equal(t[r], t[rows[0]]) for r in rows) and list(rows) == sorted(rows)
        copies = (t == t[rows[0]]).all(1).nonzero()[0]
        assert copies.tolist() == list(rows)                           # and no further copy
        halves = {(r // 32, (r >> 2) & 1) for r in rows}               # (tile, half of the wave)
        same_tile_both_halves += any((tile, 1 - h) in halves for tile, h in halves)
    assert same_tile_both_halves >= 3
    assert sum(len({r // 32 for r in rows}) > 1 for rows in km.PLANTED_GROUPS) >= 3
    idx, dist = km.knn2(q, t)
    for g, rows in enumerate(km.PLANTED_GROUPS):
        sel = group == g
        assert sel.sum() == km.PLANTED_PER_GROUP
        assert np.all(idx[sel] == rows[:2]) and np.all(dist[sel, 0] == dist[sel, 1])
        assert (dist[sel, 0] == 0).sum() == 2 and (dist[sel, 0] > 0).sum() == 4
        assert (np.any(q[sel][:, None, :] != t[rows[0]], axis=2)).sum() == 4
    assert np.all(dist[group < 0] > 100)


def test_offset_rows_rank_inside_the_proofs_slack():
    """Rows of 200 + {0, 1, 2} (and 200 + [0, 2)): the fourth and the second smallest d2 of
    every query are far closer than KNN_EPS (|q|^2 + max |t|^2) ~ 4e-5 * 2 * 128 * 201^2 = 414,
    so ``second <= floor_d2`` cannot hold for any query: all of them are rescanned."""
    for gen in (km.offset_int, km.offset_float):
        q, t = gen()
        assert q.shape[0] == km.OFFSET_NQ > 64 and t.shape[0] > km.KNN_KEEP
        s = km.sorted_d2(km.exact_d2(q, t), km.KNN_KEEP)
        spread, slack = float((s[:, 3] - s[:, 1]).max()), float(km.proof_slack(q, t).min())
        print(f"{gen.__name__}: 4th - 2nd smallest d2 at most {spread:g}, slack at least {slack:.0f}")
        assert slack > 400 and spread <= 16 and spread < slack / 25
    q, t = km.offset_float()
    assert np.any(q != np.round(q)) and q.min() >= 200 and q.max() < 202


def test_offset_tail_answers_lie_past_the_rescans_first_pass():
    """1030 offset rows: every query is inside the proof's slack, so all are rescanned, and the
    answers of queries 0 .. 4 hold rows >= 1024, which a rescanning wave reaches only in the second
    pass of its loop (4 * 256 waves) - in first place, in second place, both, and tied with row 5."""
    q, t = km.offset_tail()
    assert q.shape[0] == km.TAIL_NQ > 64 and km.TAIL_FROM < t.shape[0] == km.TAIL_NT
    d2 = km.exact_d2(q, t)
    s = km.sorted_d2(d2, km.KNN_KEEP)
    assert float((s[:, 3] - s[:, 1]).max()) < float(km.proof_slack(q, t).min()) / 3
    idx, dist = km.knn2(q, t, d2)
    assert idx[0].tolist() == [1024, 1027] and dist[0].tolist() == [0.0, 0.0]
    assert idx[1, 0] == 1025 and idx[2, 0] == 1026 and idx[4, 0] == 1029
    assert idx[3].tolist() == [5, 1028] and dist[3, 0] == dist[3, 1] > 0
    assert np.all(idx[1:3, 1] < km.TAIL_FROM) and np.all(idx[5:] < km.TAIL_FROM)
