"""Local alignment without a GPU: the properties of the contract's NumPy model
(tests/flow_model.py) that the device is later held to - the nesting of the levels, the counts and
sums, the eligibility edge, the tie and hysteresis rules, the lower median -, the workspace formula,
the record against the C compiler, the command line, the recovery of planted shifts, the meeting
of the two patches, the invariants of the apply, and five faults that each break a check."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest

import flow_cases as fc
import flow_model as fm
from conftest import ROOT
from pano360_amd import _lib, flow, stitcher


@contextlib.contextmanager
def fault(name):
    fm.FAULTS.add(name)
    try:
        yield
    finally:
        fm.FAULTS.discard(name)


# -------------------------------------------------------- the model's own properties
def direct_sample(g0, v0, level, Y, X):
    """Sample (Y, X) of a level from its own 2^l x 2^l tile of level 0 alone."""
    g = g0[Y << level:(Y + 1) << level, X << level:(X + 1) << level].astype(np.int64)
    v = v0[Y << level:(Y + 1) << level, X << level:(X + 1) << level]
    for _ in range(level):
        g = (g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2] + 2) >> 2
        v = v[0::2, 0::2] & v[0::2, 1::2] & v[1::2, 0::2] & v[1::2, 1::2]
    return int(g[0, 0]), bool(v[0, 0])


@pytest.mark.parametrize("name", ("three-130x257", "swapped-130x257"))
def test_levels_nest_on_the_mosaic_grid(name):
    patches, shape, _ = fc.case(name)
    for patch in patches:
        pyr = fm.pyramid(patch, shape, 4)
        g0, v0 = pyr[0]
        assert g0.shape == (144, 272) and not g0[~v0].any()
        y0, x0, h, w = fm.rect_of(patch)
        inside = np.zeros_like(v0)
        inside[y0:y0 + h, x0:x0 + w] = ~patch[1]
        assert np.array_equal(v0, inside)
        for level in range(1, 5):
            g, v = pyr[level]
            assert g.shape == (144 >> level, 272 >> level)
            for Y in range(g.shape[0]):
                for X in range(g.shape[1]):
                    assert (int(g[Y, X]), bool(v[Y, X])) == direct_sample(g0, v0, level, Y, X)


def test_grey_values():
    warped = np.zeros((1, 4, 4), np.float32)
    warped[0, :, :3] = [[1, 1, 1], [0, 0, 0], [1, 0, 0], [0.5, 0.25, 0.75]]
    g, v = fm.grey_of(warped, np.array([[False, False, False, True]]))
    # uint8(255 * 0.5) = 127, uint8(255 * 0.25) = 63, uint8(255 * 0.75) = 191: masked, so 0
    assert g.tolist() == [[255, 0, (255 + 2) >> 2, 0]] and v.tolist() == [[True, True, True, False]]
    g, _ = fm.grey_of(warped, np.zeros((1, 4), bool))
    assert g[0, 3] == (127 + 2 * 63 + 191 + 2) >> 2
    swapped = warped.copy()
    swapped[..., [0, 2]] = warped[..., [2, 0]]
    assert np.array_equal(fm.grey_of(swapped, np.zeros((1, 4), bool))[0], g)


@pytest.mark.parametrize("name", ("three-130x257", "level0-67x300"))
def test_counts_and_sums_against_a_per_sample_loop(name):
    _, stages = fc.model_of(name)
    rng = np.random.default_rng(5)
    for q, pair in enumerate(stages["pairs"]):
        pi, pj = stages["pyramids"][pair[0]], stages["pyramids"][pair[1]]
        for level in range(pair[2] + 1):
            by0, bx0, nby, nbx = fm.block_range(pair, level)
            vec = rng.integers(-3, 4, (nby, nbx, 2))
            n, S = fm.sums(pi[level][0], pi[level][1], pj[level][0], pj[level][1], by0, bx0, nby, nbx, vec)
            (gi, vi), (gj, vj) = pi[level], pj[level]
            hh, ww = gi.shape
            for by, bx in {(0, 0), (nby - 1, nbx - 1), (nby // 2, nbx // 2)}:
                for k, (dx, dy) in enumerate(fm.CANDIDATES):
                    cnt = tot = 0
                    for r in range(16):
                        for c in range(16):
                            y, x = 16 * (by0 + by) + r, 16 * (bx0 + bx) + c
                            yy, xx = y + vec[by, bx, 1] + dy, x + vec[by, bx, 0] + dx
                            if not (y < hh and x < ww and 0 <= yy < hh and 0 <= xx < ww):
                                continue
                            if vi[y, x] and vj[yy, xx]:
                                cnt += 1
                                tot += abs(int(gi[y, x]) - int(gj[yy, xx]))
                    assert (int(n[k, by, bx]), int(S[k, by, bx])) == (cnt, tot), (q, level, by, bx, k)


def test_candidate_order():
    assert fm.CANDIDATES == [(0, 0), (-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]


def edge_patches():
    """Two textured patches of 64 x 64 at the origin, the same content: block (0, 0) of camera 0
    has exactly 128 valid pixels, block (0, 1) 127."""
    img = fc.scene(64, 64, 31)
    mask = np.zeros((64, 64), bool)
    mask[8:16, 0:32] = True
    mask[7, 31] = True
    rect = (0, 0, 64, 64)
    return [fc.patch(fc.cut(img, rect), 0, 0, mask), fc.patch(fc.cut(img, rect), 0, 0)], (64, 64)


def edge_known():
    patches, shape = edge_patches()
    _, stages = fm.align(patches, shape, fm.Params(0), want_stages=True)
    assert [p[:3] for p in stages["pairs"]] == [(0, 1, 0)]
    return stages["levels"][0][0][..., 2]


def test_eligibility_edge():
    known = edge_known()
    assert known[0, 0] == 1 and known[0, 1] == 0 and known[1:].all()


def test_decide_ties_and_hysteresis():
    def run(n, S, gain=16):
        w, known = fm.decide(np.array(n, np.int64).reshape(9, 1), np.array(S, np.int64).reshape(9, 1), gain)
        return int(w[0]), bool(known[0])
    n = [256] * 9
    assert run(n, [100] * 9) == (0, True)                           # all tie: the centre is first
    assert run(n, [400, 50, 50, 50, 50, 50, 50, 50, 50]) == (1, True)   # the first of the minima
    # a move must gain `gain` / 16 grey levels per sample: 16 S(w) + gain n <= 16 S(c)
    assert run(n, [1000, 1000, 1000 - 256, 1000, 1000, 1000, 1000, 1000, 1000]) == (2, True)
    assert run(n, [1000, 1000, 1000 - 255, 1000, 1000, 1000, 1000, 1000, 1000]) == (0, True)
    assert run(n, [1000, 1000, 1000 - 255, 1000, 1000, 1000, 1000, 1000, 1000], gain=15) == (2, True)
    # the means are compared exactly, by cross product: 100 / 200 < 129 / 256
    assert run([256, 200] + [0] * 7, [129 + 256, 100] + [0] * 7, gain=1)[0] == 1
    # an ineligible centre: the winner stands; nothing eligible: unknown
    assert run([127, 128] + [0] * 7, [0, 5000] + [0] * 7) == (1, True)
    assert run([127] * 9, [0] * 9) == (0, False)


@pytest.mark.parametrize("name", fc.ZERO_FIELDS + ("planted-2",))
def test_flat_striped_and_identical_patches_stay(name):
    if name == "planted-2":
        patches, shape, params = fc.planted(2, (0, 0))
    else:
        patches, shape, params = fc.case(name)
    out, stages = fm.align(list(patches), shape, params, want_stages=True)
    assert stages["pairs"]
    for levels, smooth in zip(stages["levels"], stages["fields"]):
        assert all(not lv[..., :2].any() for lv in levels) and not smooth.any()
        assert levels[0][..., 2].any()
    for got, want in zip(out, patches):
        assert got[0].tobytes() == want[0].tobytes()
    assert not any(m.any() for m in stages["moved"])


def test_lower_median_against_sort():
    rng = np.random.default_rng(7)
    for m in range(1, 10):
        for _ in range(20):
            values = [int(v) for v in rng.integers(-4, 5, m)]
            assert fm.lower_median(values) == int(np.sort(values)[(m - 1) >> 1])
    assert fm.lower_median([3, -1]) == -1 and fm.lower_median([2, 2, 5, 7]) == 2


def test_smoothing_rules():
    vec = np.zeros((3, 4, 4), np.int16)
    vec[..., 2] = 1
    vec[1, 1, :2] = (9, -9)                             # an outlier among known blocks goes
    vec[0, 3] = (5, 5, 0, 0)                            # unknown, 3 known neighbours: their median
    vec[2, 3, 2] = 0
    out = fm.smooth(vec)
    assert out[1, 1].tolist() == [0, 0] and out[0, 3].tolist() == [0, 0]
    lone = np.zeros((3, 3, 4), np.int16)
    lone[0, 0] = (4, 4, 1, 0)
    lone[0, 1] = (2, 6, 1, 0)
    out = fm.smooth(lone)
    assert out[0, 0].tolist() == [2, 4] and out[1, 1].tolist() == [0, 0]    # two known: (0, 0)
    assert out[2, 2].tolist() == [0, 0]


# --------------------------------------------------- the package against the model
def host_table(patches):
    from pano360_amd import engine
    rec = np.zeros(len(patches), engine.PATCH_DTYPE)
    for k, p in enumerate(patches):
        y0, x0, h, w = fm.rect_of(p)
        pitch = (w + 3) & ~3
        rec[k] = (256, 256, 0, 0, y0, x0, h, w, 0, 0, h, w, 0, 0, h, w, pitch, pitch, k, 0)
    return rec


@pytest.fixture(scope="module")
def native():
    _lib.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    fn = handle.pano_flow_work_bytes
    fn.restype, fn.argtypes = _lib._SIGNATURES["pano_flow_work_bytes"]
    return fn


@pytest.mark.parametrize("name", fc.CASES)
def test_pairs_and_workspace_formula(name, native):
    patches, shape, params = fc.case(name)
    rects = [fm.rect_of(p) for p in patches]
    mine = flow.FlowParams(params.levels, params.gain, params.min_overlap)
    assert flow.pairs_for(rects, mine) == fm.pairs_for(rects, params)
    lay = flow.Layout(rects, mine)
    for q, pair in enumerate(lay.pairs):
        for level in range(pair[2] + 1):
            assert flow.block_range(pair, level) == fm.block_range(pair, level)
            assert lay.vec[q, level][1:] == fm.block_range(pair, level)[2:]
    for (c, level), (_, rows, cols, y0, x0) in lay.gv.items():
        assert (y0, x0, rows, cols) == fm.box_of(rects[c], level)
    rec = host_table(patches)
    got = native(rec.ctypes.data_as(ctypes.POINTER(_lib.Patch)), len(rec), shape[0], shape[1],
                 ctypes.byref(mine.native()))
    assert got == lay.total and got % 256 == 0
    want = sum(2 * r * c for _, r, c, _, _ in lay.gv.values())
    assert lay.pyramid_bytes == want and lay.vectors_at == -(-want // 256) * 256


def test_pairs_levels_and_the_63_pixel_intersection():
    rects = [fm.rect_of(p) for p in fc.case("four-67x300")[0]]
    assert [p[:3] for p in flow.pairs_for(rects)] == [(1, 2, 1), (2, 3, 1)]
    assert [p[:3] for p in flow.pairs_for(rects, flow.FlowParams(3, 16, 32))] == [(0, 1, 0), (1, 2, 1), (2, 3, 1)]
    big = [(0, 0, 600, 600), (0, 88, 600, 600)]
    assert flow.pairs_for(big)[0][:3] == (0, 1, 3) and flow.pairs_for(big, flow.FlowParams(4))[0][2] == 4
    assert flow.pairs_for([(0, 0, 128, 128), (0, 0, 128, 128)])[0][2] == 2
    assert flow.pairs_for([(0, 0, 127, 300), (0, 0, 127, 300)])[0][2] == 1


def test_refusals_of_the_workspace_size(native):
    patches, shape, _ = fc.case("four-67x300")
    rec = host_table(patches)
    ptr = rec.ctypes.data_as(ctypes.POINTER(_lib.Patch))

    def size(n=4, H=shape[0], W=shape[1], params=(3, 16, 64), table=ptr):
        return native(table, n, H, W, ctypes.byref(_lib.FlowParams(*params, 0)))
    assert size() > 0
    assert size(n=1) == 0 and size(params=(5, 16, 64)) == 0 and size(params=(-1, 16, 64)) == 0
    assert size(params=(3, 0, 64)) == 0 and size(params=(3, 4081, 64)) == 0 and size(params=(3, 16, 15)) == 0
    assert size(W=299) == 0 and size(table=None) == 0
    windowed = rec.copy()
    windowed["vw"][2] -= 4
    assert size(table=windowed.ctypes.data_as(ctypes.POINTER(_lib.Patch))) == 0


def test_the_record_against_the_c_compiler(tmp_path):
    src, exe = str(tmp_path / "rec.c"), str(tmp_path / "rec")
    fields = [f for f, _ in _lib.FlowParams._fields_]
    with open(src, "w") as fid:
        fid.write('#include <stdio.h>\n#include "pano360.h"\nint main(void)\n{\n'
                  'printf("%zu", sizeof(pano_flow_params));\n'
                  + "".join(f'printf(" %zu", __builtin_offsetof(pano_flow_params, {f}));\n' for f in fields)
                  + 'printf(" %d %d %d\\n", PANO_FLOW_MAX_LEVELS, PANO_FLOW_MIN_COUNT, PANO_FLOW_MAX_GAIN);\n'
                    "return 0;\n}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    seen = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert seen == [16, 0, 4, 8, 12, 4, 128, 4080]
    assert ctypes.sizeof(_lib.FlowParams) == 16
    assert [getattr(_lib.FlowParams, f).offset for f in fields] == [0, 4, 8, 12]
    assert (_lib.FLOW_MAX_LEVELS, _lib.FLOW_MIN_COUNT, _lib.FLOW_MAX_GAIN) == (fm.MAX_LEVELS, fm.MIN_COUNT, 4080)


def test_params():
    p = flow.FlowParams()
    assert (p.levels, p.gain, p.min_overlap, p.reach) == (3, 16, 64, 15)
    assert flow.FlowParams(0).reach == 1 and flow.FlowParams(4).reach == 31
    for bad in (dict(levels=5), dict(levels=-1), dict(levels=1.5), dict(gain=0), dict(gain=4081),
                dict(min_overlap=15)):
        with pytest.raises(ValueError):
            flow.FlowParams(**bad)
    import flow as shim
    assert shim.FlowParams is flow.FlowParams and shim.align_device is flow.align_device


def test_command_line(capsys):
    plain = stitcher.parse_args(["dir"])
    assert not hasattr(plain, "local_align") and not hasattr(plain, "local_align_levels")
    assert stitcher.local_align_of(plain) is None
    args = stitcher.parse_args(["dir", "--local-align"])
    assert args.local_align is True and not hasattr(args, "local_align_levels")
    assert repr(stitcher.local_align_of(args)) == "FlowParams(3, 16, 64)"
    args = stitcher.parse_args(["dir", "--local-align", "--local-align-levels", "0", "-b", "seam"])
    assert stitcher.local_align_of(args).levels == 0
    assert stitcher.cache_name(args) == stitcher.cache_name(plain)
    for bad in (["dir", "--local-align-levels", "2"], ["dir", "--local-align", "--local-align-levels", "5"],
                ["dir", "--local-align", "--local-align-levels", "-1"]):
        with pytest.raises(SystemExit):
            stitcher.parse_args(bad)
    assert "--local-align" in capsys.readouterr().err


def test_statistics_and_the_reach_warning(caplog):
    import logging
    rects = [(0, 0, 103, 107)] * 2
    lay = flow.Layout(rects, flow.FlowParams(1))
    host = np.zeros(lay.total, np.uint8)
    vec = lay.vectors_of(host, 0, 0)
    vec[..., 2] = 1
    vec[:2, :, 0] = 3                                   # 14 of 49 known blocks at the reach 3
    lay.field_of(host, 0)[:2, :, 0] = 3
    stats = flow.statistics(lay, host, np.array([500, 2000, 0, 0], np.int32), flow.FlowParams(1))
    assert stats == {"pairs": 1, "blocks": 49, "known": 49, "median": 0.0, "largest": 3.0, "at_reach": 14,
                     "moved": 500, "valid": 2000, "reach": 3}
    with caplog.at_level(logging.INFO):
        flow.log_statistics(stats)
    assert "1 pairs" in caplog.text and "0.2500 of the valid pixels moved" in caplog.text
    assert "further apart" in caplog.text
    caplog.clear()
    stats["at_reach"] = 4
    with caplog.at_level(logging.INFO):
        flow.log_statistics(stats)
    assert "further apart" not in caplog.text


# ------------------------------------------------------------- recovery and meeting
def misses():
    out = []
    for level, vector in fc.PLANTS:
        patches, shape, params = fc.planted(level, vector)
        _, stages = fm.align(list(patches), shape, params, want_stages=True)
        (pair,) = stages["pairs"]
        assert pair[2] == level
        inner = fc.interior_blocks(pair, level)
        assert inner.sum() >= 25
        vec = stages["levels"][0][0]
        hit = (vec[..., 0] == vector[0]) & (vec[..., 1] == vector[1]) & (vec[..., 2] == 1)
        if not hit[inner].all():
            out.append((level, vector))
    return out


def test_planted_vectors_are_recovered():
    """The level-0 block vectors, before the smoothing, equal the planted vector on every block
    wholly inside the overlap and at least the reach from its border - for all plants but the
    listed ones, at most an eighth of them."""
    assert len(fc.PLANTS) == 36
    assert {v for l, v in fc.PLANTS if l == 3} >= {(0, 0), (15, 15), (-15, 15), (15, 0), (0, -15)}
    assert frozenset(misses()) == fc.NOT_RECOVERED
    assert 8 * len(fc.NOT_RECOVERED) <= len(fc.PLANTS)


def grey_difference(a, b, level):
    """Mean |g_a - g_b| over the overlap's interior (the reach and a block from its border)."""
    ga, gb = fm.grey_of(a[0], a[1])[0].astype(np.int64), fm.grey_of(b[0], b[1])[0].astype(np.int64)
    m = fm.reach(level) + 16
    return float(np.abs(ga - gb)[m:-m, m:-m].mean())


def meeting_ratios():
    out = {}
    for level, vector in fc.PLANTS:
        if (level, vector) in fc.NOT_RECOVERED or max(abs(vector[0]), abs(vector[1])) < 2:
            continue
        patches, shape, params = fc.planted(level, vector)
        a, b = fm.align(list(patches), shape, params)
        out[level, vector] = grey_difference(a, b, level) / grey_difference(patches[0], patches[1], level)
    return out


def test_the_patches_meet():
    ratios = meeting_ratios()
    print({k: round(v, 3) for k, v in ratios.items()})
    assert len(ratios) >= 20
    assert all(r < 1 for r in ratios.values()), ratios


# --------------------------------------------------------------------- invariants
def check_invariants(patches, out, stages):
    pairs = stages["pairs"]
    for c, (src, got) in enumerate(zip(patches, out)):
        assert got[1] is src[1] and got[2] is src[2]
        partners = [p[1] if p[0] == c else p[0] for p in pairs if c in p[:2]]
        if not partners:
            assert got is src
            continue
        y0, x0, h, w = fm.rect_of(src)
        covered, weighted = np.zeros((h, w), bool), np.zeros((h, w), bool)
        for j in partners:
            jy, jx, jh, jw = fm.rect_of(patches[j])
            a0, a1, b0, b1 = max(y0, jy), min(y0 + h, jy + jh), max(x0, jx), min(x0 + w, jx + jw)
            part = ~patches[j][1][a0 - jy:a1 - jy, b0 - jx:b1 - jx]
            covered[a0 - y0:a1 - y0, b0 - x0:b1 - x0] |= part
            weighted[a0 - y0:a1 - y0, b0 - x0:b1 - x0] |= part & (patches[j][0][a0 - jy:a1 - jy, b0 - jx:b1 - jx, 3] > 0)
        same = (got[0].view(np.uint32) == src[0].view(np.uint32)).all(axis=2)
        assert same[~covered].all() and same[src[1]].all()
        dx, dy = stages["disp"][c]
        assert not dx[~weighted].any() and not dy[~weighted].any()
        assert not stages["moved"][c][~weighted].any()


@pytest.mark.parametrize("name", fc.CASES)
def test_invariants_of_the_apply(name):
    patches, _, _ = fc.case(name)
    out, stages = fc.model_of(name)
    check_invariants(patches, out, stages)
    if name not in fc.ZERO_FIELDS:
        assert sum(int(m.sum()) for m in stages["moved"]) > 1000


def test_a_vector_at_the_reach_and_three_cameras_on_a_pixel():
    _, stages = fc.model_of("four-67x300")
    assert any((np.abs(f) == 3).any() for f in stages["fields"])
    patches, _, _ = fc.case("three-130x257")
    assert [p[2] for p in fc.model_of("three-130x257")[1]["pairs"]] == [1, 2, 2]
    assert [p[2] for p in fc.model_of("capped-130x257")[1]["pairs"]] == [1, 1, 1]
    assert fc.model_of("level0-67x300")[1]["pairs"][0][:3] == (0, 1, 0)
    cover = np.zeros((130, 257), int)
    for warped, mask, where in patches:
        cover[where] += ~mask
    assert (cover == 3).sum() > 5000
    assert any(p[1].any() for p in patches) and any(p[0].shape[1] % 4 for p in patches)


# -------------------------------------------------------------------------- faults
def test_fault_sign():
    with fault("sign"):
        ratios = meeting_ratios()
    assert any(r >= 1 for r in ratios.values())


def test_fault_alpha():
    patches, shape, params = fc.case("four-67x300")
    with fault("alpha"):
        out, stages = fm.align(list(patches), shape, params, want_stages=True)
    with pytest.raises(AssertionError):
        check_invariants(patches, out, stages)


def test_fault_gain():
    patches, shape, params = fc.case("flat-67x300")
    with fault("gain"):
        _, stages = fm.align(list(patches), shape, params, want_stages=True)
    assert any(f.any() for f in stages["fields"])


def test_fault_count():
    with fault("count"):
        assert edge_known()[0, 1] == 1


def test_fault_median():
    with fault("median"):
        assert fm.lower_median([3, -1]) == 3
        vec = np.zeros((1, 2, 4), np.int16)
        vec[0, 0], vec[0, 1] = (1, 0, 1, 0), (5, 0, 1, 0)
        assert fm.smooth(vec)[0, 0, 0] == 5
    assert fm.smooth(vec)[0, 0, 0] == 1
