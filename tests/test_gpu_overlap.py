"""GPU: ``pano_overlap_stats`` (csrc/gains.hip) on the forged cases of tests/overlap_cases.py against
the NumPy model of its contract, tests/overlap_model.py: the pixel counts by integer equality, the
two double sums within the bound of any summation order.  The native entry is called directly, with
the case's own hat tables and block width, into ``partials`` and ``stats`` filled with 0xFF bytes.
What the cases depend on is asserted on the model alone in tests/test_overlap_host.py."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_cases as oc  # noqa: E402
import overlap_model as om  # noqa: E402

pytestmark = pytest.mark.gpu

OK = 0
UNIT = 2.0 ** -53
_worst = {"ratio": -1.0, "where": None}


@functools.lru_cache(maxsize=None)
def _model(name, k):
    case = oc.CASES[name]
    minv, i, j = case.pairs[k]
    got = om.overlap(case.frames[i], case.frames[j], minv, case.bw0, case.hat_x, case.hat_y)
    return got.count, got.sum_i, got.sum_j


class _Rig:
    """Frames, hat tables and the camera table of one case on the device, with host copies of
    every input the call may not write."""

    def __init__(self, eng, frames, hat_x, hat_y):
        import torch
        from pano360_amd import engine
        self.eng = eng
        self.h, self.w = (int(v) for v in frames.shape[1:3])
        self.frames = torch.from_numpy(np.array(frames)).to(eng.device)
        self.hat_x = torch.from_numpy(np.array(hat_x, np.float64)).to(eng.device)
        self.hat_y = torch.from_numpy(np.array(hat_y, np.float64)).to(eng.device)
        rec = np.zeros(len(frames), dtype=engine.CAMERA_DTYPE)
        for k in range(len(frames)):
            rec[k] = (np.zeros(9), self.frames[k].data_ptr(), self.hat_x.data_ptr(),
                      self.hat_y.data_ptr(), self.h, self.w, 0, 0, 0, 0)
        self.cams = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(eng.device)
        self.nblk = int(eng.lib.pano_overlap_blocks(self.h, self.w))
        assert self.nblk == -(-self.h // oc.TILE_H) * -(-self.w // oc.TILE_W)
        self.inputs = dict(frames=self.frames, hat_x=self.hat_x, hat_y=self.hat_y, cams=self.cams,
                           lut255=eng.lut255)
        self.before = {key: t.cpu().numpy().tobytes() for key, t in self.inputs.items()}

    def call(self, pairs, bw0, n_pairs=None, h=None, w=None, null=()):
        """pano_overlap_stats into poisoned outputs sized for ``pairs`` (for one pair where there
        is none): (status, stats as float64 [pairs][3])."""
        import torch
        from pano360_amd import _lib, engine
        eng = self.eng
        table = np.zeros(max(len(pairs), 1), dtype=engine.PAIR_DTYPE)
        for k, rec in enumerate(pairs):
            table[k] = rec
        rows = len(table)
        dev_pairs = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(eng.device)
        partials = torch.full((rows * self.nblk * 24,), 0xFF, dtype=torch.uint8, device=eng.device)
        stats = torch.full((rows * 24,), 0xFF, dtype=torch.uint8, device=eng.device)
        ptr = dict(cams=self.cams, pairs=dev_pairs, lut255=eng.lut255, partials=partials,
                   stats=stats)
        ptr = {key: None if key in null else _lib._ptr(t) for key, t in ptr.items()}
        status = eng.lib.pano_overlap_stats(
            eng.ctx(), ptr["cams"], ptr["pairs"], len(pairs) if n_pairs is None else n_pairs,
            self.h if h is None else h, self.w if w is None else w, bw0, ptr["lut255"],
            ptr["partials"], ptr["stats"])
        torch.cuda.synchronize()
        assert dev_pairs.cpu().numpy().tobytes() == table.tobytes()
        self.last_partials = partials.cpu().numpy()
        return status, stats.cpu().numpy().view(np.float64).reshape(rows, 3)

    def assert_inputs_unwritten(self):
        for key, t in self.inputs.items():
            assert t.cpu().numpy().tobytes() == self.before[key], key


def _rig(eng, name):
    case = oc.CASES[name]
    return _Rig(eng, case.frames, case.hat_x, case.hat_y)


def _poisoned(stats):
    return bool(np.all(stats.view(np.uint8) == 0xFF))


def _assert_model(stats_row, name, k):
    count, sum_i, sum_j = _model(name, k)
    assert stats_row[0] == count, (name, k, stats_row[0], count)
    for got, want, which in ((stats_row[1], sum_i, "frame i"), (stats_row[2], sum_j, "frame j")):
        # any order of summing 3 count non-negative doubles stays within (3 count - 1) 2^-53 of
        # their sum, relatively; the model's fsum is that sum rounded once
        bound = 3 * count * UNIT * want
        if count == 0:
            assert got == 0.0 and np.signbit(got) == 0, (name, k, which)
            continue
        ratio = abs(got - want) / bound
        if ratio > _worst["ratio"]:
            _worst.update(ratio=ratio, where=(name, k, which))
        assert abs(got - want) <= bound, (name, k, which, got, want, ratio)


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_counts_and_sums_equal_the_model(eng, name):
    case = oc.CASES[name]
    rig = _rig(eng, name)
    status, stats = rig.call(case.pairs, case.bw0)
    assert status == OK
    for k in range(len(case.pairs)):
        _assert_model(stats[k], name, k)
    rig.assert_inputs_unwritten()


def test_largest_error_against_the_bound():
    print(f"largest |sum - fsum| / (3 count 2^-53 sum) over {len(oc.CASES)} cases: "
          f"{_worst['ratio']:.3g} at {_worst['where']}")
    assert _worst["where"] is not None


# ----------------------------------------------------------------------------------- batches
BATCH_CASE = "size_17x130_engine"


def _batch_pairs():
    """The case's own pairs, pairs with j < i and i == j, a horizon, a zero denominator, and
    footprints that leave every tile, or every tile but some, skipped."""
    case = oc.CASES[BATCH_CASE]
    persp = case.pairs[1][0]
    extra = [(persp, 2, 0), (oc.IDENTITY, 1, 1), (persp, 2, 1),
             (oc.CASES["horizon_along_a_column_ones"].pairs[0][0], 1, 2),
             (oc.CASES["zero_den_at_pixel_70_9_ones"].pairs[0][0], 2, 0),
             (oc.translation(1000, 0), 0, 1), (oc.translation(-63 - 1 / 128, 0), 0, 2),
             (oc.scaling(4.0, -256.0, -64.0), 1, 0)]
    return list(case.pairs) + [(oc._mat(m), i, j) for m, i, j in extra]


def test_a_batch_equals_its_pairs_one_by_one(eng):
    case = oc.CASES[BATCH_CASE]
    rig = _rig(eng, BATCH_CASE)
    pairs = _batch_pairs()
    assert any(j < i for _, i, j in pairs) and any(i == j for _, i, j in pairs)
    alone = []
    for pair in pairs:
        status, stats = rig.call([pair], case.bw0)
        assert status == OK
        alone.append(stats[0].tobytes())
        minv, i, j = pair
        want = om.overlap(case.frames[i], case.frames[j], minv, case.bw0, case.hat_x, case.hat_y)
        assert stats[0, 0] == want.count
    assert len(set(alone)) >= len(pairs) - 2
    for order in (list(range(len(pairs))), list(range(len(pairs)))[::-1]):
        runs = []
        for _ in range(3):
            status, stats = rig.call([pairs[k] for k in order], case.bw0)
            assert status == OK
            runs.append(stats.tobytes())
            for row, k in enumerate(order):
                assert stats[row].tobytes() == alone[k], (order[0], k)
        assert runs[0] == runs[1] == runs[2]
    rig.assert_inputs_unwritten()


def test_a_skipped_tile_writes_zeros(eng):
    """Every tile skipped: the poison in ``partials`` is gone, the sums are +0."""
    rig = _rig(eng, oc.CULL_ALL)
    case = oc.CASES[oc.CULL_ALL]
    status, stats = rig.call(case.pairs, case.bw0)
    assert status == OK and not stats.any() and not np.signbit(stats).any()
    assert not rig.last_partials.any()


# ----------------------------------------------------------------------------------- n_pairs
FOUR = ([1, 0, 0, 0, 1, 0, 0, 0, 1], [1, 0, 3 / 64, 0, 1, 5 / 64, 0, 0, 1],
        [0.5, 0, 0.25, 0, 0.5, 0.25, 0, 0, 1], [1, 0, 0.5, 0, 1, 0.25, 0, 0, 1])


def _tiny_rig(eng):
    frames = np.random.default_rng(11).integers(0, 256, (2, 2, 2, 3), dtype=np.uint8)
    return _Rig(eng, frames, np.ones(2), np.ones(2)), frames


def test_no_pairs_is_ok_and_writes_nothing(eng):
    rig, _ = _tiny_rig(eng)
    status, stats = rig.call([], 2)
    assert status == OK and _poisoned(stats) and np.all(rig.last_partials == 0xFF)


def test_65535_pairs_in_one_call(eng):
    rig, frames = _tiny_rig(eng)
    pairs = [(oc._mat(FOUR[k % 4]), k % 2, (k // 2) % 2) for k in range(4)]
    want = []
    for minv, i, j in pairs:
        got = om.overlap(frames[i], frames[j], minv, 2, np.ones(2), np.ones(2))
        want.append((got.count, got.sum_i, got.sum_j))
    assert [c for c, _, _ in want] == [1, 1, 4, 1] and len(set(want)) == 4
    status, stats = rig.call(pairs * 16383 + pairs[:3], 2)
    assert status == OK and len(stats) == 65535
    for k in range(4):
        rows = stats[k::4]
        assert np.all(rows == rows[0]), k
        count, sum_i, sum_j = want[k]
        assert rows[0, 0] == count
        for got, exact in ((rows[0, 1], sum_i), (rows[0, 2], sum_j)):
            assert abs(got - exact) <= 3 * count * UNIT * exact


def test_65536_pairs_are_refused(eng):
    """Every buffer has the size the arguments claim: a missing refusal reads nothing out of
    bounds and fails here."""
    from pano360_amd import _lib
    rig, _ = _tiny_rig(eng)
    pairs = [(oc._mat(FOUR[k % 4]), 0, 1) for k in range(4)] * 16384
    status, stats = rig.call(pairs, 2)
    assert len(stats) == 65536 and status != OK and _poisoned(stats)
    assert b"65536" in _lib.lib().pano_last_error()


# --------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(eng):
    from pano360_amd import _lib
    case = oc.CASES[BATCH_CASE]
    rig = _rig(eng, BATCH_CASE)
    pairs = list(case.pairs)
    refused = [dict(null=(key,)) for key in ("cams", "pairs", "lut255", "partials", "stats")]
    refused += [dict(h=1), dict(h=0), dict(w=1), dict(w=-3), dict(bw0=0), dict(bw0=-64),
                dict(n_pairs=-1)]
    for kw in refused:
        bw0 = kw.pop("bw0", case.bw0)
        status, stats = rig.call(pairs, bw0, **kw)
        assert status != OK and _poisoned(stats), kw
        assert np.all(rig.last_partials == 0xFF), kw
        assert len(_lib.lib().pano_last_error()) > 10, kw
    # 32768 rows or columns, every buffer as large as the arguments claim
    for h, w in ((32768, 2), (2, 32768)):
        big = _Rig(eng, np.zeros((2, h, w, 3), np.uint8), np.ones(w), np.ones(h))
        status, stats = big.call([(oc.IDENTITY, 0, 1)], 64)
        assert status != OK and _poisoned(stats), (h, w)
        assert b"32768" in _lib.lib().pano_last_error()
    status, stats = rig.call(pairs, case.bw0)
    assert status == OK
    for k in range(len(pairs)):
        _assert_model(stats[k], BATCH_CASE, k)
    rig.assert_inputs_unwritten()


# ----------------------------------------------------------------------------------- engine
def test_engine_one_pair_per_call_equals_the_default(eng):
    from pano360_amd import engine, synth
    n, w, h = 6, 130, 17
    rots, intrs = synth.make_cameras(n, w, h, sweep_deg=150.0, jitter=0.02, seed=3)
    imgs = np.random.default_rng(17).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    frames = eng.upload_frames(list(imgs))
    default = eng.equalize_gains(frames, rots, intrs)
    single = eng.equalize_gains(frames, rots, intrs, chunk_bytes=1)
    for a, b in zip(default[:3], single[:3]):
        assert a.tobytes() == b.tobytes()
    assert default[3].cpu().numpy().tobytes() == single[3].cpu().numpy().tobytes()
    pairs = engine.overlap_pairs(rots, intrs, w, h)
    assert len(pairs) >= 3
    sizes, overlaps = np.zeros((n, n)), np.zeros((n, n))
    for rec in pairs:
        i, j = int(rec["i"]), int(rec["j"])
        got = om.overlap(imgs[i], imgs[j], rec["minv"], oc.warp_bw0(h, w), oc.hat(w), oc.hat(h))
        sizes[i, j] = sizes[j, i] = got.count
        if got.count:
            overlaps[i, j] = got.sum_i / (3.0 * got.count)
            overlaps[j, i] = got.sum_j / (3.0 * got.count)
    assert np.array_equal(default[1], sizes) and (sizes > 0).sum() >= 6
    # the engine rounds its mean to float32 once
    np.testing.assert_allclose(default[0], overlaps, rtol=2.0 ** -24 + 1e-12, atol=0)
