"""Bracket alignment without a GPU: the properties of the contract's NumPy model
(tests/align_model.py) that the device is later held to, the level count, the workspace formula
and the refusals that need no GPU, the command line and the cache names, and the recovery of
planted shifts by the model on every case of tests/align_cases.py."""
import numpy as np
import pytest

import align_cases
import align_model
from pano360_amd import align, fuse


# -------------------------------------------------------- the model's own properties
@pytest.mark.parametrize("shape", [(128, 192), (131, 200), (67, 129)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_levels_nest(shape):
    """A 64 x 64-aligned tile of level 0 determines its part of every level up to 6 (and a
    128 x 128-aligned one up to 7): the pyramid of a tile alone is the tile of the pyramid."""
    frame = align_cases.random_stack(shape[0], shape[1], 1, 3)[0]
    for tile, levels in ((64, 6), (128, 7)):
        whole = align_model.pyramid(frame, levels)
        for y0 in range(0, shape[0], tile):
            for x0 in range(0, shape[1], tile):
                part = align_model.pyramid(frame[y0:y0 + tile, x0:x0 + tile], levels)
                for l, (a, b) in enumerate(zip(whole, part)):
                    want = a[y0 >> l:(y0 + tile) >> l, x0 >> l:(x0 + tile) >> l]
                    # (a tile cut by the frame's edge may keep a pixel the frame's level drops)
                    assert np.array_equal(b[:want.shape[0], :want.shape[1]], want), (tile, y0, x0, l)
        assert [g.shape for g in whole] == [(shape[0] >> l, shape[1] >> l) for l in range(levels + 1)]


def test_grey_and_down_values():
    frame = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 2, 3]]], np.uint8)
    assert align_model.grey(frame).tolist() == [[255, 0, 29, 149, 77, (29 + 300 + 231 + 128) >> 8]]
    g = np.array([[0, 1, 255, 255, 9], [1, 1, 255, 254, 9], [7, 7, 7, 7, 7]], np.uint8)
    assert align_model.down(g).tolist() == [[1, 255]]   # (3 + 2) >> 2, (1019 + 2) >> 2; odd row, column dropped


def test_median_against_sort():
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 4, 5, 64, 255, 1000):
        for hi in (1, 2, 256):
            g = rng.integers(0, hi, n, dtype=np.uint8)
            assert align_model.median(g) == int(np.sort(g)[(n + 1) // 2 - 1]), (n, hi)
    assert align_model.median(np.array([0, 255], np.uint8)) == 0
    assert align_model.median(np.full(7, 255, np.uint8)) == 255


def test_packing_round_trips():
    rng = np.random.default_rng(12)
    for h, w in ((1, 1), (3, 31), (2, 32), (5, 33), (4, 64), (3, 129)):
        bits = rng.integers(0, 2, (h, w)).astype(bool)
        words = align_model.pack(bits)
        assert words.dtype == np.uint32 and words.shape == (h, (w + 31) // 32)
        assert np.array_equal(align_model.unpack(words, w), bits)
        for y, x in ((0, 0), (h - 1, w - 1), (h // 2, w // 2)):
            assert bool(words[y, x >> 5] >> (x & 31) & 1) == bits[y, x]
        if w % 32:                                      # the padding bits are 0
            assert not (words[:, -1] >> (w % 32)).any()
    g = np.array([[10, 14, 15, 5, 6, 9]], np.uint8)
    tb, eb = align_model.bitmaps(g, 10, 4)
    assert tb.tolist() == [[0b000110]] and eb.tolist() == [[0b001100]]


def test_err_against_a_dense_evaluation():
    rng = np.random.default_rng(13)
    h, w = 9, 37
    a_t, a_e, b_t, b_e = (rng.integers(0, 2, (h, w)).astype(bool) for _ in range(4))
    for cx, cy in ((0, 0), (1, 0), (-1, 0), (0, 1), (3, -2), (-5, 4), (36, 8), (37, 0), (0, -9), (-40, 3)):
        want = 0
        for y in range(h):
            for x in range(w):
                if 0 <= y - cy < h and 0 <= x - cx < w:
                    want += int((a_t[y, x] ^ b_t[y - cy, x - cx]) & a_e[y, x] & b_e[y - cy, x - cx])
        assert align_model.err(a_t, a_e, b_t, b_e, cx, cy) == want, (cx, cy)


def test_the_tie_rule_and_the_candidate_order():
    assert align_model.CANDIDATES == ((0, 0), (-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
    for case in align_cases.CASES:
        kind, h, w, k, r = case
        m = align_cases.model_of(case)
        if kind == "identical":                         # every count of (0, 0) is 0: it wins
            assert not m["shifts"].any() and not m["err"][:, :, 0].any()
        if kind == "flat":                              # an empty eb: every count is 0
            assert not np.concatenate([e.ravel() for e in m["eb"][0]]).any()
            assert not (m["shifts"][0].any() if r != 0 else m["shifts"].any())
            assert not (m["err"][0].any() if r != 0 else m["err"].any())
        if kind == "extremes":                          # g > m is empty for a frame of one value
            assert not m["shifts"][0].any() and not m["shifts"][-1].any()
        assert not m["shifts"][r].any() and not m["err"][r].any()
        assert np.abs(m["shifts"]).max() <= align_cases.reach_of(h, w)


def test_apply_replicates_the_border():
    frame = np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3)
    out = align_model.apply(frame, 2, -1)
    for y in range(4):
        for x in range(5):
            assert np.array_equal(out[y, x], frame[min(max(y + 1, 0), 3), min(max(x - 2, 0), 4)])
    assert np.array_equal(align_model.apply(frame, 0, 0), frame)


# ------------------------------------------------------------------ levels
def test_levels_for():
    want = {1: 0, 15: 0, 16: 0, 31: 0, 32: 1, 63: 1, 64: 2, 127: 2, 128: 3, 256: 4, 1024: 6, 2047: 6,
            2048: 6, 32767: 6}
    for side, levels in want.items():
        assert align.levels_for(side, 5000) == align.levels_for(5000, side) == levels, side
        assert align_model.levels_for(side, 5000) == levels
        assert levels == 0 or side >> levels >= 16      # the coarsest level's short side
    assert align.levels_for(2048, 4096, 7) == 7 and align.levels_for(2047, 4096, 7) == 6
    assert align.levels_for(300, 500, 3) == 3 and align.levels_for(300, 500, 0) == 0
    assert [align_cases.levels_of(h, w) for h, w in align_cases.SIZES + (align_cases.BIG,)] == [0, 0, 1, 1, 2, 3, 4]
    assert align.reach_for(301, 517) == 31 and align.reach_for(16, 16) == 1


def test_params_and_stacks_are_checked_before_any_device_work():
    p = align.AlignParams()
    assert (p.max_bits, p.exclude, p.reference) == (6, 4, None)
    assert [p.reference_of(k) for k in (2, 3, 8)] == [1, 1, 4]
    for bad in ({"max_bits": -1}, {"max_bits": 8}, {"exclude": -1}, {"exclude": 128}, {"reference": -1}):
        with pytest.raises(ValueError):
            align.AlignParams(**bad)
    a = np.zeros((4, 5, 3), np.uint8)
    for bad in ([[a]], [[a] * 9], [[a, np.zeros((4, 6, 3), np.uint8)]], [[a, a.astype(np.float32)]],
                [[a, np.zeros((4, 5), np.uint8)]], [[a[..., :2], a[..., :2]]]):
        for call in (align.shifts_device, align.align_device):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError, match="reference"):
        align.shifts_device([[a, a]], align.AlignParams(reference=2))


def test_top_level_module_serves_the_package():
    import align as top
    assert top.align_device is align.align_device and top.AlignParams is align.AlignParams
    assert top.shifts_device is align.shifts_device and top.levels_for is align.levels_for


# ---------------------------------------------------------------- workspace
def _work_bytes(h, w, k):
    """The documented formula (include/pano360.h)."""
    def a256(n):
        return -(-n // 256) * 256
    lm = align.levels_for(h, w, 7)
    total = a256(1024 * k * (lm + 1)) + a256(36 * k * (lm + 1)) + a256(4 * k * (lm + 1))
    for l in range(lm + 1):
        hl, wl = h >> l, w >> l
        total += k * (a256(hl * ((wl + 3) // 4 * 4)) + a256(8 * hl * ((wl + 31) // 32)))
    return total


def test_work_bytes_formula():
    from pano360_amd import _lib
    lib = _lib.lib()
    for h, w, k in ((1, 1, 2), (16, 16, 2), (17, 33, 8), (67, 129, 3), (301, 517, 3), (2160, 3840, 3),
                    (32767, 32767, 8), (1, 32767, 2)):
        assert lib.pano_align_work_bytes(h, w, k) == _work_bytes(h, w, k), (h, w, k)
    assert _work_bytes(1, 1, 2) == 2048 + 256 + 256 + 2 * (256 + 256)
    for bad in ((0, 4, 2), (4, 0, 2), (32768, 4, 2), (4, 32768, 2), (4, 4, 1), (4, 4, 9)):
        assert lib.pano_align_work_bytes(*bad) == 0, bad


def test_stack_limits():
    assert align.MAX_EXPOSURES == 8 and align.MAX_SIDE == 32767


# ------------------------------------------------------------ command line
def test_command_line_of_the_stitcher():
    import stitcher
    from test_fuse_host import TODAY_STITCHER
    args = stitcher.parse_args(["DIR"])
    assert vars(args) == TODAY_STITCHER                 # the namespace it was
    assert not fuse.align_of(args) and fuse.from_args(args) is None
    assert stitcher.cache_name(args) == "DIR_s2"
    plain = stitcher.parse_args(["DIR", "--bracket", "3"])
    assert "bracket_align" not in vars(plain) and "bracket_align_bits" not in vars(plain)
    assert stitcher.cache_name(plain) == "DIR_s2_b3" and fuse.from_args(plain).align is None
    chosen = stitcher.parse_args(["DIR", "--bracket", "3", "--bracket-align"])
    assert chosen.bracket_align is True and "bracket_align_bits" not in vars(chosen)
    assert stitcher.cache_name(chosen) == "DIR_s2_b3a"
    b = fuse.from_args(chosen)
    assert b.k == 3 and (b.align.max_bits, b.align.exclude, b.align.reference) == (6, 4, None)
    full = stitcher.parse_args(["DIR", "--bracket", "5", "--bracket-align", "--bracket-align-bits", "3",
                                "--detector", "msop", "--lens", "cal.json"])
    assert stitcher.cache_name(full) == "DIR_s2_msop_b5a_lens"
    assert fuse.from_args(full).align.max_bits == 3
    for bad in (["--bracket-align"], ["--bracket-align-bits", "3"],
                ["--bracket", "3", "--bracket-align-bits", "3"],
                ["--bracket", "3", "--bracket-align", "--bracket-align-bits", "8"],
                ["--bracket", "3", "--bracket-align", "--bracket-align-bits", "-1"],
                ["--bracket", "3", "--bracket-align", "--bracket-align-bits", "x"],
                ["--bracket", "3", "--bracket-align", "--bracket-align-bits"]):
        with pytest.raises(SystemExit) as err:
            stitcher.parse_args(["DIR"] + bad)
        assert err.value.code == 2, bad


def test_command_line_of_features():
    from pano360_amd import features
    args = features.parse_args(["--path", "some/DIR"])
    assert vars(args) == {"path": "some/DIR", "detector": "sift", "lens": None, "lens_interp": None,
                          "lens_focal": None}
    assert features.cache_name(args) == "DIR"
    assert features.cache_name(features.parse_args(["--path", "some/DIR", "--bracket", "3"])) == "DIR_b3"
    chosen = features.parse_args(["--path", "some/DIR", "--bracket", "3", "--bracket-align", "--detector", "msop"])
    assert features.cache_name(chosen) == "DIR_msop_b3a"
    for bad in (["--bracket-align"], ["--bracket", "3", "--bracket-align-bits", "2"]):
        with pytest.raises(SystemExit) as err:
            features.parse_args(bad)
        assert err.value.code == 2, bad


def test_bracket_carries_the_alignment():
    assert fuse.Bracket(3).align is None
    how = align.AlignParams(max_bits=2)
    assert fuse.Bracket(3, None, how).align is how and fuse.Bracket(3, align=how).align is how


# ------------------------------------------------------------------ recovery
def test_the_model_recovers_every_planted_shift():
    """A condition on the inputs, not a tolerance: the model returns exactly the planted shift on
    every recovery case, and the cases left out are exactly the ones it misses.  368 of the 400
    plants are kept (figures of this recipe: tests/align_cases.py)."""
    cases = align_cases.recovery_cases()
    assert len(cases) == 368 and len(align_cases.NOT_RECOVERED) == 32
    sizes = {(c[0], c[1]) for c in cases}
    assert sizes == set(align_cases.SIZES + (align_cases.BIG,))
    for h, w in sizes:                                  # the offsets the issue lists, where in reach
        offs = align_cases.offsets_of(h, w)
        big = min(align_cases.reach_of(h, w), min(h, w) // 8)
        assert {(0, 0), (1, 0), (-1, 0), (big, big), (-big, big), (big, -big)} <= set(offs)
        assert ((3, -2) in offs) == (align_cases.reach_of(h, w) >= 3)
        assert ((-5, 4) in offs) == (align_cases.reach_of(h, w) >= 5)
    for case in cases:
        h, w, _, _, off = case
        found = align_model.shifts(align_cases.recovery_stack(case), 0, align_cases.max_bits_of(h, w))
        assert tuple(int(v) for v in found[1]) == off and not found[0].any(), case
    for case in align_cases.NOT_RECOVERED:
        h, w, _, _, off = case
        found = align_model.shifts(align_cases.recovery_stack(case), 0, align_cases.max_bits_of(h, w))
        assert tuple(int(v) for v in found[1]) != off, case


def test_the_planted_cases_of_the_gpu_tests_are_recovered():
    for case in align_cases.CASES:
        if case[0] == "planted":
            want = align_cases.planted_offsets(case)
            assert want[case[4]] == (0, 0) and len(want) == case[3]
            assert align_cases.model_of(case)["shifts"].tolist() == [list(o) for o in want], case
            aligned, _ = align_model.align(align_cases.stack_of(case), case[4],
                                           align_cases.max_bits_of(case[1], case[2]))
            assert any(not np.array_equal(a, f) for a, f in zip(aligned, align_cases.stack_of(case)))
