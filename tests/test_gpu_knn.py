"""GPU: ``pano_knn2`` (csrc/knn.hip) against the NumPy model of its contract, tests/knn_model.py,
bit for bit: the same two rows (equal distances: lower index first) and the same float32
distances, whether a query's answer was proven from the matrix cores' ranking or rescanned.
This file has no tolerances.  What the cases depend on is asserted on the model alone in
tests/test_knn_host.py."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_model as km  # noqa: E402

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -1
SWEEP_D = (1, 5, 16, 17, 63, 64, 65, 100, 127, 128)


def _unit_peak(rows):
    """Each set divided by its largest magnitude: the peak of either is exactly 1."""
    return tuple(np.ascontiguousarray(r / np.abs(r).max()) for r in rows)


CASES = {
    "sift128": lambda: km.sift_like(),
    "sift64": lambda: km.sift_like(d=64, seed=1),
    "uniform_int128": lambda: km.uniform_int(300, 700, 128, 31),
    "uniform_int64": lambda: km.uniform_int(300, 700, 64, 32),
    "signed_int128": lambda: km.signed_int(300, 700, 128, 33),
    "signed_int64": lambda: km.signed_int(300, 700, 64, 34),
    "planted": lambda: km.planted()[:2],
    "offset_int": km.offset_int,
    "offset_float": km.offset_float,
    "offset_tail": km.offset_tail,
    "uniform": lambda: km.uniform_float(700, 1333, 128, 35),
    "unit": lambda: km.unit_float(),
    "normal": lambda: km.normal_float(400, 900, 128, 36),
    "edges": lambda: km.sift_like(257, 1025, 128, seed=2),
    "meta_float": lambda: km.unit_float(257, 600, 128, seed=37, planted_rows=100),
    "peak1_uniform": lambda: _unit_peak(km.uniform_float(150, 400, 128, 38)),
    "peak1_normal": lambda: _unit_peak(km.normal_float(150, 400, 128, 39)),
}
for _d in SWEEP_D:
    CASES[f"uniform_d{_d}"] = functools.partial(km.uniform_float, 70, 101, _d, 40 + _d)
    CASES[f"normal_d{_d}"] = functools.partial(km.normal_float, 70, 101, _d, 200 + _d)
    CASES[f"unit_d{_d}"] = functools.partial(km.unit_float, 70, 101, _d, 400 + _d, 30)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(query, train, d2 of the model), computed once and read-only."""
    q, t = CASES[name]()
    d2 = km.exact_d2(q, t)
    for a in (q, t, d2):
        a.setflags(write=False)
    return q, t, d2


def _model(name):
    q, t, d2 = _case(name)
    return km.knn2(q, t, d2)


def _run(eng, q, t, scale=None):
    """``features.knn2_device``: (idx int64 [nq][2], dist float32 [nq][2], rescans) on the host."""
    import torch
    from pano360_amd import features
    idx, dist, rescans = features.knn2_device(
        torch.from_numpy(np.array(q)).to(eng.device),
        torch.from_numpy(np.array(t)).to(eng.device), eng=eng, want_rescans=True,
        scale=scale)
    return idx.cpu().numpy(), dist.cpu().numpy(), rescans


def _assert_same(got, want, what):
    """idx equal and dist equal as bits."""
    (gi, gd), (wi, wd) = got[:2], want[:2]
    assert gi.shape == wi.shape and gd.shape == wd.shape and gd.dtype == np.float32, what
    bad = np.nonzero(np.any(gi != wi, axis=1) | np.any(gd.view(np.uint32) != wd.view(np.uint32),
                                                       axis=1))[0]
    if len(bad):
        r = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(gi)} queries differ, the first is {r}: "
                             f"idx {gi[r].tolist()} dist {gd[r].tolist()}, the model has "
                             f"{wi[r].tolist()} {wd[r].tolist()}")


def _check(eng, name, scale=None):
    q, t, _ = _case(name)
    got = _run(eng, q, t, scale)
    _assert_same(got, _model(name), name)
    return got


@pytest.mark.parametrize("name", ["sift128", "sift64", "uniform_int128", "uniform_int64",
                                  "signed_int128", "signed_int64"])
def test_integer_valued_rows(eng, name):
    """a. Rows as OpenCV's SIFT gives them (Poisson(3): 25 queries tie first / second and 37
    second / third at d = 128), uniform 0..255 and signed -127..127, d = 128 and 64: squared
    distances are exact integers."""
    rescans = _check(eng, name)[2]
    print(f"knn2 {name}: {rescans} rescans")


def test_planted_ties(eng):
    """b. Groups of 2, 3, 5 and 6 identical train rows, inside one tile on both halves of the
    wave and across tiles; queries equal to the row or a few integer steps away: the two lowest
    rows of the group, and the candidate list of four cannot prove that (25 of the 76 queries
    were rescanned on the MI355X)."""
    q, t, group = km.planted()
    idx, dist, rescans = _check(eng, "planted")
    for g, rows in enumerate(km.PLANTED_GROUPS):
        assert np.all(idx[group == g] == rows[:2])
        assert (dist[group == g] == 0).all(1).sum() == 2
    print(f"knn2 planted: {rescans} rescans of {len(q)} queries")
    assert rescans > 0


@pytest.mark.parametrize("name", ["offset_int", "offset_float"])
def test_whole_set_inside_the_ranking_noise(eng, name):
    """c. Rows of 200 + {0, 1, 2} and of 200 + [0, 2): the fourth smallest d2 is within 16 of
    the second while the proof needs 414, so every query is rescanned - more queries than the
    rescan grid has rows (64), so its stride loop runs.  With the fractional rows the ranked
    order is really wrong (the product errs by more than neighbours differ: with KNN_EPS = 0 the
    kernel returned 8 wrong rows of 150).  The run showed 150 rescans of 150 on both."""
    rescans = _check(eng, name)[2]
    print(f"knn2 {name}: {rescans} rescans of {km.OFFSET_NQ} queries")
    assert rescans > 64
    assert rescans == km.OFFSET_NQ


def test_rescan_reaches_rows_past_its_first_pass(eng):
    """e. 1030 offset rows, every query rescanned, and the nearest rows of queries 0 .. 4 are rows
    1024 .. 1029 (tests/test_knn_host.py): the second pass of a rescanning wave's loop over
    ``train`` (4 * 256 waves), a tie between its two passes included."""
    idx, _, rescans = _check(eng, "offset_tail")
    print(f"knn2 offset_tail: {rescans} rescans of {km.TAIL_NQ} queries")
    assert idx[0].tolist() == [1024, 1027] and idx[3].tolist() == [5, 1028]
    assert rescans == km.TAIL_NQ


@pytest.mark.parametrize("name", ["uniform", "unit", "normal"])
def test_float_rows(eng, name):
    """d. Uniform rows, unit-norm RootSIFT-like rows with planted near duplicates, signed
    standard-normal rows (MSOP-like), d = 128."""
    rescans = _check(eng, name)[2]
    print(f"knn2 {name}: {rescans} rescans")


@pytest.mark.parametrize("d", SWEEP_D)
def test_feature_counts(eng, d):
    """d. 70 x 101 rows of every kind at feature counts on both sides of the switch between
    four and eight k-steps (64 | 65) and ragged ones (zero padding inside a k-step)."""
    for kind in ("uniform", "normal", "unit"):
        _check(eng, f"{kind}_d{d}")


EDGE_NQ = (1, 31, 32, 33, 127, 128, 129, 257)
EDGE_NT = (2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 1025)


def _edge(eng, nq, nt):
    q, t, d2 = _case("edges")
    want = km.knn2(q[:nq], t[:nt], d2[:nq, :nt])
    _assert_same(_run(eng, q[:nq], t[:nt]), want, f"{nq} queries against {nt} rows")


@pytest.mark.parametrize("nt", (5, 65, 1025))
def test_query_count_edges(eng, nt):
    """e. Dead waves and dead tiles in the last block of the ranking kernel."""
    for nq in EDGE_NQ:
        _edge(eng, nq, nt)


@pytest.mark.parametrize("nq", (1, 33, 129))
def test_train_count_edges(eng, nq):
    """e. Padding rows with +inf norms, no more rows than the candidate list holds, and one row
    past the 1024 waves of the rescan."""
    for nt in EDGE_NT:
        _edge(eng, nq, nt)


@pytest.mark.parametrize("name", ["meta_float", "edges"])
def test_scaling_by_a_power_of_two(eng, name):
    """f. Both sets times 2^20 and 2^-20: the scale the caller derives moves with the data, the
    packed halves are the same - the same rows, distances scaled exactly, as many rescans."""
    q, t, _ = _case(name)
    idx, dist, rescans = _check(eng, name)
    for factor in (np.float32(2.0 ** 20), np.float32(2.0 ** -20)):
        got = _run(eng, q * factor, t * factor)
        _assert_same(got, (idx, dist * factor), f"{name} x {factor}")
        assert got[2] == rescans


@pytest.mark.parametrize("name", ["meta_float", "edges"])
def test_permuted_train_rows(eng, name):
    """f. Ties follow the new indices, not the old rows."""
    q, t, d2 = _case(name)
    perm = np.random.default_rng(50).permutation(len(t))
    want = km.knn2(q, t[perm], d2[:, perm])
    _assert_same(_run(eng, q, t[perm]), want, f"{name} permuted")
    if name == "edges":
        assert np.any(want[0] != perm.argsort()[_model(name)[0]])    # some tie did change rows


@pytest.mark.parametrize("name", ["meta_float", "edges"])
def test_a_query_does_not_depend_on_its_neighbours(eng, name):
    """f. Queries [37:70] and [128:129] alone: the bytes they had inside the full call."""
    q, t, _ = _case(name)
    idx, dist, _ = _check(eng, name)
    for lo, hi in ((37, 70), (128, 129)):
        _assert_same(_run(eng, q[lo:hi], t), (idx[lo:hi], dist[lo:hi]), f"{name} [{lo}:{hi}]")


@pytest.mark.parametrize("name", ["meta_float", "edges", "offset_int"])
def test_two_calls_give_the_same_bytes(eng, name):
    """f. Also where every query goes through the rescan's atomic minima."""
    q, t, _ = _case(name)
    first, second = _run(eng, q, t), _run(eng, q, t)
    _assert_same(second, first, f"{name} again")
    assert first[2] == second[2]


def test_explicit_scale_on_integer_rows(eng):
    """g. Uniform 0..255 at scales 2^-10 .. 8 (peak 2040 of the 2048 the header allows): the
    same bytes."""
    for scale in (2.0 ** -10, 0.25, 1.0, 4.0, 8.0):
        _check(eng, "uniform_int128", scale)


@pytest.mark.parametrize("name", ["peak1_uniform", "peak1_normal"])
def test_explicit_scale_at_both_ends_of_the_rule(eng, name):
    """g. Float rows whose largest magnitude is exactly 1, in both sets: ``scale`` = 2048, the
    header's upper end, and 2^-3, its lower end, where nearly every low half is a float16
    denormal; the answer is the exact one at both (and in between)."""
    q, t, _ = _case(name)
    assert np.abs(q).max() == 1.0 and np.abs(t).max() == 1.0
    for scale in (2048.0, 1.0, 0.125):
        rescans = _check(eng, name, scale)[2]
        print(f"knn2 {name} at scale {scale}: {rescans} rescans")


# ------------------------------------------------------------------------- the native entry

SENTINEL_IDX, SENTINEL_DIST = -77, 7.25


def _native(eng, q, t, nq=None, nt=None, d=None, scale=1.0, null=(), work_fill=0xFF,
            with_rescans=True, ctx=True):
    """pano_knn2 into prefilled outputs: (status, idx, dist, rescans) on the host."""
    import torch
    from pano360_amd import _lib
    dev = dict(query=torch.from_numpy(np.array(q)).to(eng.device),
               train=torch.from_numpy(np.array(t)).to(eng.device))
    size = int(eng.lib.pano_knn2_work_bytes(len(q), len(t), q.shape[1]))
    assert size > 0
    dev["work"] = torch.full((size,), work_fill, dtype=torch.uint8, device=eng.device)
    dev["idx"] = torch.full((len(q), 2), SENTINEL_IDX, dtype=torch.int32, device=eng.device)
    dev["dist"] = torch.full((len(q), 2), SENTINEL_DIST, dtype=torch.float32, device=eng.device)
    dev["rescans"] = torch.full((1,), SENTINEL_IDX, dtype=torch.int32, device=eng.device)
    ptr = {key: None if key in null else _lib._ptr(v) for key, v in dev.items()}
    status = eng.lib.pano_knn2(
        eng.ctx() if ctx else None, ptr["query"], len(q) if nq is None else nq, ptr["train"],
        len(t) if nt is None else nt, q.shape[1] if d is None else d, C.c_float(scale),
        ptr["work"], ptr["idx"], ptr["dist"], ptr["rescans"] if with_rescans else None)
    torch.cuda.synchronize()
    return (status, dev["idx"].cpu().numpy(), dev["dist"].cpu().numpy(),
            int(dev["rescans"].item()))


def _untouched(out):
    return (np.all(out[1] == SENTINEL_IDX) and np.all(out[2] == np.float32(SENTINEL_DIST))
            and out[3] == SENTINEL_IDX)


def test_native_entry_ignores_what_the_scratch_held(eng):
    """h. Scratch of 0xFF and of 0x00 bytes: every output row written, the same bytes, the
    model's; ``rescans`` may be null."""
    q, t, _ = _case("planted")
    want = _model("planted")
    outs = [_native(eng, q, t, scale=2.0, work_fill=fill) for fill in (0xFF, 0x00)]
    outs.append(_native(eng, q, t, scale=2.0, with_rescans=False))
    for out in outs:
        assert out[0] == OK
        _assert_same(out[1:3], want, "native entry")
    assert outs[0][3] == outs[1][3] > 0 and outs[2][3] == SENTINEL_IDX


def test_native_entry_without_queries(eng):
    """h. nq = 0: PANO_OK and nothing written."""
    q, t, _ = _case("planted")
    out = _native(eng, q, t, nq=0)
    assert out[0] == OK and _untouched(out)


def test_native_entry_refusals(eng):
    """h. PANO_EINVAL and the outputs as they were; a valid call on the same context then gives
    the right answer."""
    q, t, _ = _case("planted")
    refused = [dict(nt=0), dict(nt=1), dict(nt=-5), dict(nq=-1), dict(d=0), dict(d=129),
               dict(d=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")),
               dict(scale=float("inf")), dict(scale=float("-inf")), dict(ctx=False)]
    refused += [dict(null=(key,)) for key in ("query", "train", "work", "idx", "dist")]
    for kw in refused:
        out = _native(eng, q, t, **kw)
        assert out[0] == EINVAL, kw
        assert _untouched(out), kw
    out = _native(eng, q, t, scale=2.0)
    assert out[0] == OK
    _assert_same(out[1:3], _model("planted"), "after the refusals")
