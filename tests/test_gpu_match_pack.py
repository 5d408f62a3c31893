"""GPU: pano_match_pack (match_pack_kernel, csrc/ransac.hip) called through its native entry,
against the NumPy model of its contract (ransac_model.pack) bit for bit: the sizes around the
wave's 64 and the block's 1024 lanes crossed with survivor patterns, the comparison on forged
boundary distances, train indices out of range, the buffers around a pair's region, refusals,
and the packing over ``knn2_device`` against ``flann_matching`` (whose host ratio test is also
checked here on 1-d descriptors that put the float32 distances on the boundary).

Every keypoint has coordinates of its own, (q + 0.25, -q) for query q and (1000 + t, t + 0.5) for
train row t, so a row of pts names its (q, t).  Outputs are prefilled with a sentinel: the kernel
writes the survivors' rows and nothing else."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_model as rm  # noqa: E402

pytestmark = pytest.mark.gpu

NT = 97
GUARD = 64                                   # sentinel rows kept after a pair's nq rows
SENT_F = np.float32(-12345.5)
SENT_I = np.int32(-12345)
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 37)
PATTERNS = ("none", "all", "alternate", "lane63", "lane0", "one_in_last_chunk", "random30")
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def _keypoints(nq, nt):
    q, t = np.arange(nq, dtype=np.float32), np.arange(nt, dtype=np.float32)
    return (np.stack([q + np.float32(0.25), -q], axis=1),
            np.stack([t + np.float32(1000), t + np.float32(0.5)], axis=1))


def _pattern(name, nq, rng):
    q = np.arange(nq)
    if name == "none":
        return np.zeros(nq, bool)
    if name == "all":
        return np.ones(nq, bool)
    if name == "alternate":
        return q % 2 == 0
    if name == "lane63":
        return q % 64 == 63
    if name == "lane0":
        return q % 64 == 0
    if name == "one_in_last_chunk":          # the chunks before it half full, then one survivor
        last = (nq - 1) // 1024 * 1024
        keep = (rng.random(nq) < 0.5) & (q < last)
        keep[nq - 1] = True
        return keep
    return rng.random(nq) < 0.3


def _forge(keep, rng, nt=NT):
    """(idx, dist) whose ratio test at 0.7 passes exactly where `keep`: d0 = 0.5 d1 or 0.9 d1, a
    valid nearest row, garbage in the second neighbour's index."""
    nq = len(keep)
    d1 = rng.uniform(1.0, 2.0, nq).astype(np.float32)
    d0 = (d1 * np.where(keep, np.float32(0.5), np.float32(0.9))).astype(np.float32)
    idx = np.stack([rng.integers(0, nt, nq), rng.integers(INT32_MIN, INT32_MAX, nq, endpoint=True)],
                   axis=1).astype(np.int32)
    return idx, np.stack([d0, d1], axis=1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Call:
    """One pair's buffers on the device: inputs, and sentinel-filled outputs of nq + GUARD rows
    with the count between two sentinel words."""

    def __init__(self, eng, idx, dist, kq, kt):
        import torch
        self.eng, self.torch = eng, torch
        self.host = [np.ascontiguousarray(idx, np.int32).reshape(-1, 2),
                     np.ascontiguousarray(dist, np.float32).reshape(-1, 2),
                     np.ascontiguousarray(kq, np.float32).reshape(-1, 2),
                     np.ascontiguousarray(kt, np.float32).reshape(-1, 2)]
        self.nq = len(self.host[0])
        # (a spare row: a refused call with a pointer 4 bytes in would still stay inside)
        self.dev = [torch.from_numpy(np.concatenate([h, np.zeros((1, 2), h.dtype)])).to(eng.device)
                    for h in self.host]
        self.pts = torch.full((self.nq + GUARD, 4), float(SENT_F), dtype=torch.float32,
                              device=eng.device)
        self.match = torch.full((self.nq + GUARD, 2), int(SENT_I), dtype=torch.int32,
                                device=eng.device)
        self.count = torch.full((3,), int(SENT_I), dtype=torch.int32, device=eng.device)

    def args(self, nt, ratio=0.7, nq=None, null_inputs=False):
        from pano360_amd import engine
        ins = [None] * 4 if null_inputs else [engine._ptr(t) for t in self.dev]
        outs = [None, None] if null_inputs else [engine._ptr(self.pts), engine._ptr(self.match)]
        return [self.eng.ctx(), ins[0], ins[1], self.nq if nq is None else nq, C.c_double(ratio),
                ins[2], ins[3], nt, outs[0], outs[1], engine._ptr(self.count[1:])]

    def run(self, args):
        from pano360_amd import _lib
        _lib.check(self.eng.lib.pano_match_pack(*args), "pano_match_pack")

    def outputs(self):
        return (self.count.cpu().numpy(), self.pts.cpu().numpy(), self.match.cpu().numpy())

    def inputs_unchanged(self):
        return all(np.array_equal(_bits(t.cpu().numpy()[:-1]), _bits(h))
                   for t, h in zip(self.dev, self.host))

    def untouched(self):
        count, pts, match = self.outputs()
        return bool(np.all(count == SENT_I) and np.all(pts == SENT_F) and np.all(match == SENT_I))


def _check(eng, idx, dist, kq, kt, nt, ratio=0.7):
    """Run one pair and compare with the model bit for bit; returns the surviving queries."""
    call = _Call(eng, idx, dist, kq, kt)
    call.run(call.args(nt, ratio))
    count, pts, match = call.outputs()
    want_pts, want_match, k = rm.pack(idx, dist, ratio, kq, kt, nt)
    assert count.tolist() == [SENT_I, k, SENT_I]
    assert np.array_equal(match[:k], want_match), np.nonzero(match[:k] != want_match)[0][:8]
    assert np.array_equal(_bits(pts[:k]), _bits(want_pts))
    # rows count .. nq - 1 and the guard band keep the sentinel: survivors only are written
    assert np.all(pts[k:] == SENT_F) and np.all(match[k:] == SENT_I)
    assert call.inputs_unchanged()
    call.run(call.args(nt, ratio))                      # the same bytes again
    again = call.outputs()
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip((count, pts, match), again))
    return match[:k, 0]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nq", SIZES)
def test_survivor_patterns_equal_the_model(eng, nq, pattern):
    rng = np.random.default_rng(1000 * nq + PATTERNS.index(pattern))
    keep = _pattern(pattern, nq, rng)
    idx, dist = _forge(keep, rng)
    kq, kt = _keypoints(nq, NT)
    got = _check(eng, idx, dist, kq, kt, NT)
    assert np.array_equal(got, np.nonzero(keep)[0])
    if pattern == "one_in_last_chunk":
        assert np.sum(got >= (nq - 1) // 1024 * 1024) == 1


def test_no_queries_writes_a_zero_count_from_null_buffers(eng):
    empty_i, empty_f = np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float32)
    call = _Call(eng, empty_i, empty_f, empty_f, empty_f)
    call.run(call.args(NT, null_inputs=True))
    count, pts, match = call.outputs()
    assert count.tolist() == [SENT_I, 0, SENT_I]
    assert np.all(pts == SENT_F) and np.all(match == SENT_I)
    call.run(call.args(0, null_inputs=True))            # and with no train rows either
    assert call.outputs()[0].tolist() == [SENT_I, 0, SENT_I]


def test_the_comparison_is_strict_and_in_float64(eng):
    rng = np.random.default_rng(7)
    n = 400
    dist = rm.boundary_distances(rng, n)
    contract = np.arange(n) % 2 == 0
    differ = int(np.sum(rm.float32_ratio_test(dist, 0.7) != contract))
    print(f"{differ} of {n} boundary rows are decided differently by a float32 comparison")
    assert differ >= 100
    idx = np.stack([rng.integers(0, NT, n), rng.integers(INT32_MIN, INT32_MAX, n)], 1).astype(np.int32)
    kq, kt = _keypoints(n, NT)
    got = _check(eng, idx, dist, kq, kt, NT)
    assert np.array_equal(got, np.nonzero(contract)[0])

    inf, nan = np.inf, np.nan
    rows = np.array([[0.5, 1.0],            # 0  d0 == 0.5 d1 exactly: not kept at ratio 0.5
                     [0.25, 0.5],           # 1  the same, other values
                     [0.0, 0.0],            # 2  not kept
                     [3.0, inf],            # 3  kept
                     [nan, 1.0],            # 4  not kept
                     [1.0, nan],            # 5  not kept
                     [nan, nan],            # 6  not kept
                     [0.25, 1.0],           # 7  kept
                     [inf, inf],            # 8  not kept
                     [0.0, 1.0]], np.float32)       # 9  kept
    rows = np.tile(rows, (7, 1))                    # 70 rows: more than a wave
    idx = np.stack([np.arange(len(rows)) % NT, np.full(len(rows), -3)], 1).astype(np.int32)
    kq, kt = _keypoints(len(rows), NT)
    got = _check(eng, idx, rows, kq, kt, NT, ratio=0.5)
    assert np.array_equal(got % 10, np.tile([3, 7, 9], 7)) and len(got) == 21


def test_train_indices_out_of_range_never_survive(eng):
    rng = np.random.default_rng(11)
    nq = 200
    bad = np.array([-1, NT, NT + 1, INT32_MAX, INT32_MIN])
    first = rng.integers(0, NT, nq)
    first[::2] = bad[np.arange(len(first[::2])) % len(bad)]
    first[[1, 3]] = 0, NT - 1                       # the two ends of the range survive
    idx = np.stack([first, rng.integers(INT32_MIN, INT32_MAX, nq)], 1).astype(np.int32)
    dist = np.tile(np.array([[0.1, 1.0]], np.float32), (nq, 1))        # every row would pass
    kq, kt = _keypoints(nq, NT)
    got = _check(eng, idx, dist, kq, kt, NT)
    assert np.array_equal(got, np.arange(1, nq, 2))
    # no train rows at all: nothing survives
    assert len(_check(eng, idx, dist, kq, kt[:0], 0)) == 0


def test_three_pairs_back_to_back_stay_inside_their_regions(eng):
    """The layout of ``features._Pairs``: pair p packs into pts[off[p]:], match[off[p]:] and
    counts[p:].  The middle pair has 1025 queries that all survive, so its region is full and a
    row too many would land in the next pair's."""
    import torch
    from pano360_amd import _lib, engine
    rng = np.random.default_rng(3)
    sizes = (65, 1025, 300)
    keeps = [rng.random(65) < 0.5, np.ones(1025, bool), rng.random(300) < 0.3]
    off = np.concatenate([[0], np.cumsum(sizes)])
    total = int(off[-1])
    pts = torch.full((total + GUARD, 4), float(SENT_F), dtype=torch.float32, device=eng.device)
    match = torch.full((total + GUARD, 2), int(SENT_I), dtype=torch.int32, device=eng.device)
    counts = torch.full((len(sizes) + 1,), int(SENT_I), dtype=torch.int32, device=eng.device)
    want_pts, want_match = pts.cpu().numpy().copy(), match.cpu().numpy().copy()
    want_counts = counts.cpu().numpy().copy()
    for p in (1, 0, 2):
        idx, dist = _forge(keeps[p], rng)
        kq, kt = _keypoints(sizes[p], NT)
        kq = kq + np.float32(4096 * p)               # the pairs' rows differ from each other's
        dev = [torch.from_numpy(a).to(eng.device) for a in (idx, dist, kq, kt)]
        o = int(off[p])
        _lib.check(eng.lib.pano_match_pack(
            eng.ctx(), engine._ptr(dev[0]), engine._ptr(dev[1]), sizes[p], C.c_double(0.7),
            engine._ptr(dev[2]), engine._ptr(dev[3]), NT, engine._ptr(pts[o:]),
            engine._ptr(match[o:]), engine._ptr(counts[p:])), "pano_match_pack")
        m_pts, m_match, k = rm.pack(idx, dist, 0.7, kq, kt, NT)
        assert k == int(keeps[p].sum())
        want_pts[o:o + k], want_match[o:o + k], want_counts[p] = m_pts, m_match, k
        # the pair's survivors are there, and every other row and count is what it was
        assert np.array_equal(counts.cpu().numpy(), want_counts), p
        assert np.array_equal(_bits(pts.cpu().numpy()), _bits(want_pts)), p
        assert np.array_equal(match.cpu().numpy(), want_match), p
    assert want_counts.tolist() == [int(k.sum()) for k in keeps] + [SENT_I]


@pytest.mark.parametrize("fault", ["pts + 4", "dist + 4", "null count", "nq = -1", "nt = -1"])
def test_refusals_leave_the_outputs_alone(eng, fault):
    from pano360_amd import _lib
    rng = np.random.default_rng(5)
    nq = 100
    idx, dist = _forge(np.ones(nq, bool), rng)
    kq, kt = _keypoints(nq, NT)
    call = _Call(eng, idx, dist, kq, kt)
    args = call.args(NT)
    if fault == "pts + 4":
        args[8] = C.c_void_p(call.pts.data_ptr() + 4)
    elif fault == "dist + 4":
        args[2] = C.c_void_p(call.dev[1].data_ptr() + 4)
    elif fault == "null count":
        args[10] = None
    elif fault == "nq = -1":
        args[3] = -1
    else:
        args[7] = -1
    with pytest.raises(_lib.PanoError, match="pano_match_pack"):
        call.run(args)
    assert call.untouched() and call.inputs_unchanged()
    call.run(call.args(NT))                          # the same buffers are accepted as they are
    assert call.outputs()[0].tolist() == [SENT_I, nq, SENT_I]


# ------------------------------------------------------------------ with the search in front
def _descriptors(rng, nq=300, nt=400, d=128):
    """Random 128-d rows; each query is a train row plus noise of its own size, so the ratio test
    passes for some and fails for others."""
    train = rng.uniform(0, 255, (nt, d)).astype(np.float32)
    noise = rng.uniform(0, 120, (nq, 1))
    query = train[rng.integers(0, nt, nq)] + rng.normal(0, 1, (nq, d)) * noise
    return query.astype(np.float32), train


def test_packing_over_knn2_equals_flann_matching(eng):
    import torch
    from pano360_amd import engine, features
    assert eng is engine.engine()                    # flann_matching runs on the process's engine
    rng = np.random.default_rng(21)
    query, train = _descriptors(rng)
    idx, dist = features.knn2_device(torch.from_numpy(query).to(eng.device),
                                     torch.from_numpy(train).to(eng.device))
    idx = idx.to(torch.int32).cpu().numpy()
    kq, kt = _keypoints(len(query), len(train))
    got = _check(eng, idx, dist.cpu().numpy(), kq, kt, len(train), ratio=features.LOWE_RATIO)
    listed = [(m.queryIdx, m.trainIdx) for m in features.flann_matching(query, train)]
    assert [(int(q), int(idx[q, 0])) for q in got] == listed
    assert 30 <= len(listed) <= len(query) - 30      # both outcomes occur


def test_flann_matching_keeps_what_the_float64_comparison_keeps(eng):
    """One 1-d query at 0 against train rows x and y: y has 11 mantissa bits, so its distance is
    y exactly; x is float32(0.7 y) or a float32 neighbour of it, so the nearest distance sits on
    the boundary of the ratio test.  The keep-set is defined from the float32 distances of
    ``knn2_device`` compared in float64."""
    import torch
    from pano360_amd import features
    rng = np.random.default_rng(9)
    n = 600
    y = (rng.integers(1024, 2048, n) * 2.0 ** (rng.integers(-3, 4, n) - 10)).astype(np.float32)
    x = (0.7 * y.astype(np.float64)).astype(np.float32)
    side = np.arange(n) % 3
    x = np.where(side == 1, np.nextafter(x, np.float32(-np.inf)),
                 np.where(side == 2, np.nextafter(x, np.float32(np.inf)), x)).astype(np.float32)
    query = np.zeros((1, 1), np.float32)
    dists, kept = np.zeros((n, 2), np.float32), np.zeros(n, bool)
    for k in range(n):
        train = np.array([[x[k]], [y[k]]], np.float32)
        idx, dist = features.knn2_device(torch.from_numpy(query).to(eng.device),
                                         torch.from_numpy(train).to(eng.device))
        assert idx.cpu().numpy().tolist() == [[0, 1]]
        dists[k] = dist.cpu().numpy()[0]
        found = features.flann_matching(query, train)
        assert len(found) <= 1
        kept[k] = len(found) == 1
        if found:
            assert (found[0].queryIdx, found[0].trainIdx) == (0, 0)
            assert found[0].distance == float(dists[k, 0])
    assert np.array_equal(dists[:, 1], y)
    want = dists[:, 0].astype(np.float64) < 0.7 * dists[:, 1].astype(np.float64)
    differ = int(np.sum(rm.float32_ratio_test(dists, 0.7) != want))
    print(f"{differ} of {n} cases are decided differently by a float32 comparison; "
          f"{int(want.sum())} kept")
    assert differ >= 100
    assert np.array_equal(kept, want), np.nonzero(kept != want)[0][:10]
