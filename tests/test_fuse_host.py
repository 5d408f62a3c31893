"""Exposure fusion without a GPU: the level count, the file grouping, the command line and the
cache names, the workspace formula, and the properties of the contract's NumPy model
(tests/fuse_model.py) that the device is later held to."""
import numpy as np
import pytest

import fuse_cases
import fuse_model
from pano360_amd import fuse


# ------------------------------------------------------------------ levels
def test_levels_for():
    want = {1: 0, 2: 0, 3: 0, 4: 1, 5: 1, 6: 1, 7: 1, 8: 2, 9: 2, 4095: 10, 4096: 11, 4097: 11}
    for side, levels in want.items():
        assert fuse.levels_for(side, 5000) == fuse.levels_for(5000, side) == levels, side
        assert fuse_model.levels_for(side, 5000) == levels
        # the coarsest level stays at least 2 wide where there is one: pyrUp is defined on it
        coarse = side
        for _ in range(levels):
            coarse = (coarse + 1) // 2
        assert levels == 0 or coarse >= 2
    assert [fuse.levels_for(h, w) for h, w in fuse_cases.SIZES] == [0, 0, 0, 1, 1, 3, 4, 5]


# ---------------------------------------------------------------- grouping
def test_group_files():
    files = ["p2_c.jpg", "p1_b.jpg", "p2_a.jpg", "p1_a.jpg", "p1_c.jpg", "p2_b.jpg"]
    assert fuse.group_files(files, 3) == [["p1_a.jpg", "p1_b.jpg", "p1_c.jpg"],
                                          ["p2_a.jpg", "p2_b.jpg", "p2_c.jpg"]]
    assert fuse.group_files(files, 2) == [["p1_a.jpg", "p1_b.jpg"], ["p1_c.jpg", "p2_a.jpg"],
                                          ["p2_b.jpg", "p2_c.jpg"]]
    assert fuse.group_files([], 3) == []
    with pytest.raises(ValueError, match="5 images"):
        fuse.group_files(files[:5], 3)
    for bad in (1, 9):
        with pytest.raises(ValueError):
            fuse.group_files(files, bad)


def test_params_are_checked():
    p = fuse.FuseParams()
    assert (p.contrast, p.saturation, p.exposure, p.n_levels) == (1.0, 1.0, 1.0, None)
    for bad in ({"contrast": -1}, {"saturation": float("nan")}, {"exposure": float("inf")},
                {"n_levels": -1}):
        with pytest.raises(ValueError):
            fuse.FuseParams(**bad)


def test_fuse_device_refuses_bad_stacks_before_any_device_work():
    a = np.zeros((4, 5, 3), np.uint8)
    for bad in ([[a]], [[a] * 9], [[a, np.zeros((4, 6, 3), np.uint8)]], [[a, a.astype(np.float32)]],
                [[a, np.zeros((4, 5), np.uint8)]], [[a[..., :2], a[..., :2]]]):
        with pytest.raises(ValueError):
            fuse.fuse_device(bad)
    with pytest.raises(ValueError, match="n_levels"):
        fuse.fuse_device([[a, a]], fuse.FuseParams(n_levels=2))


# ------------------------------------------------------------ command line
TODAY_STITCHER = {'path': 'DIR', 'shrink': 2, 'ba': 'incr', 'equalize': False, 'crop': False,
                  'blend': 'multiband', 'ghost_tol': None, 'out': None, 'register': False,
                  'detector': 'sift', 'view': [], 'equirect': None, 'cube': None, 'deepzoom': False,
                  'multires': None, 'tile': 512, 'fill': False, 'lens': None, 'lens_interp': None,
                  'lens_focal': None}


def test_command_line_of_the_stitcher():
    import stitcher
    args = stitcher.parse_args(["DIR"])
    assert vars(args) == TODAY_STITCHER                 # the namespace it was
    assert fuse.bracket_of(args) is None and fuse.from_args(args) is None
    assert stitcher.cache_name(args) == "DIR_s2"
    chosen = stitcher.parse_args(["DIR", "--bracket", "3"])
    assert chosen.bracket == 3 and "bracket_weights" not in vars(chosen)
    assert stitcher.cache_name(chosen) == "DIR_s2_b3"
    b = fuse.from_args(chosen)
    assert b.k == 3 and (b.params.contrast, b.params.saturation, b.params.exposure) == (1, 1, 1)
    full = stitcher.parse_args(["DIR", "--bracket", "5", "--bracket-weights", "1,0.5,0", "--detector",
                                "msop", "--lens", "cal.json"])
    assert stitcher.cache_name(full) == "DIR_s2_msop_b5_lens"
    b = fuse.from_args(full)
    assert b.k == 5 and (b.params.contrast, b.params.saturation, b.params.exposure) == (1, 0.5, 0)
    for bad in (["--bracket-weights", "1,1,1"], ["--bracket", "1"], ["--bracket", "9"],
                ["--bracket", "x"], ["--bracket"], ["--bracket", "3", "--bracket-weights", "1,1"],
                ["--bracket", "3", "--bracket-weights", "1,-1,1"],
                ["--bracket", "3", "--bracket-weights", "1,nan,1"],
                ["--bracket", "3", "--bracket-weights", "a,b,c"],
                ["--bracket", "3", "--bracket-weights"]):
        with pytest.raises(SystemExit) as err:
            stitcher.parse_args(["DIR"] + bad)
        assert err.value.code == 2, bad


def test_command_line_of_features():
    from pano360_amd import features
    args = features.parse_args(["--path", "some/DIR"])
    assert vars(args) == {"path": "some/DIR", "detector": "sift", "lens": None, "lens_interp": None,
                          "lens_focal": None}
    assert features.cache_name(args) == "DIR"
    chosen = features.parse_args(["--path", "some/DIR", "--bracket", "3", "--detector", "msop"])
    assert features.cache_name(chosen) == "DIR_msop_b3"
    assert features.cache_name(features.parse_args(["--path", "some/DIR", "--bracket", "3", "--lens",
                                                    "c.json"])) == "DIR_b3_lens"
    for bad in (["--bracket-weights", "1,1,1"], ["--bracket", "0"]):
        with pytest.raises(SystemExit) as err:
            features.parse_args(bad)
        assert err.value.code == 2, bad


def test_top_level_module_serves_the_package():
    import fuse as top
    assert top.fuse_device is fuse.fuse_device and top.FuseParams is fuse.FuseParams
    assert top.group_files is fuse.group_files and top.levels_for is fuse.levels_for


# ---------------------------------------------------------------- workspace
def _work_bytes(h, w, k):
    """The documented formula (include/pano360.h)."""
    total = 0
    for _ in range(fuse.levels_for(h, w) + 1):
        total += -(-16 * k * h * w // 256) * 256 + -(-16 * h * w // 256) * 256
        h, w = (h + 1) // 2, (w + 1) // 2
    return total


def test_work_bytes_formula():
    from pano360_amd import _lib
    lib = _lib.lib()
    for h, w, k in ((1, 1, 2), (2, 3, 8), (4, 4, 2), (67, 129, 3), (150, 270, 8), (2160, 3840, 3),
                    (32767, 32767, 8), (1, 32767, 2)):
        assert lib.pano_fuse_work_bytes(h, w, k) == _work_bytes(h, w, k), (h, w, k)
    assert _work_bytes(1, 1, 2) == 512 and _work_bytes(4, 4, 2) == 512 + 256 + 256 + 256
    for bad in ((0, 4, 2), (4, 0, 2), (32768, 4, 2), (4, 32768, 2), (4, 4, 1), (4, 4, 9)):
        assert lib.pano_fuse_work_bytes(*bad) == 0, bad


def test_stack_limits():
    from pano360_amd import _lib
    assert fuse.MAX_EXPOSURES == _lib.FUSE_MAX_EXPOSURES == 8
    assert fuse.MAX_SIDE == _lib.FUSE_MAX_SIDE == 32767


# -------------------------------------------------------- the model's own properties
@pytest.mark.parametrize("shape", fuse_cases.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_identity(shape):
    """Two identical exposures fuse to that frame exactly: the weights are exactly 0.5, the
    collapse returns (G - u) + u, within 2 ulp of G, and times 255 that is far from a tie."""
    frame = fuse_cases.random_stack(shape[0], shape[1], 1, 77)[0]
    for n_levels in (None, 0):
        fused, q = fuse_model.fuse([frame, frame], n_levels=n_levels)
        assert np.array_equal(q, frame)
        assert np.abs(fused - frame.astype(np.float32) / np.float32(255)).max() <= 4 * 2.0 ** -24


def test_model_window_scene():
    """What the feature is for: the fused frame keeps both ends of a 64 : 1 scene that the middle
    exposure clips at one end and the long exposure over half of.  Figures of this model
    (default_rng(5)): clipped share 0.0011 (middle exposure 0.168, long 0.499); standard deviation
    over the right quarter 28.3 against 16.8 for the rounded plain mean, over the left quarter
    15.6 against 8.4."""
    stack = fuse_cases.window_stack()
    _, q = fuse_model.fuse(stack)
    w = q.shape[1]
    plain = np.rint(np.mean([f.astype(np.float64) for f in stack], axis=0))
    clipped = float(((q == 0) | (q == 255)).mean())
    right = (float(q[:, -(w // 4):].astype(np.float64).std()), float(plain[:, -(w // 4):].std()))
    left = (float(q[:, :w // 4].astype(np.float64).std()), float(plain[:, :w // 4].std()))
    print(clipped, right, left)
    assert clipped < 0.01
    assert right[0] >= 1.4 * right[1]
    assert left[0] >= 1.4 * left[1]


def test_model_float32_weights_are_close_to_float64():
    """The bound of the GPU test has room: NumPy's own float32 evaluation of stage A stays within
    a small part of it."""
    worst = 0.0
    for case in fuse_cases.CASES[:8]:
        for frame in fuse_cases.stack_of(case):
            w64 = fuse_model.raw_weights(frame, np.float64)
            w32 = fuse_model.raw_weights(frame, np.float32)
            assert w32.dtype == np.float32 and np.isfinite(w32).all() and (w32 >= np.float32(1e-12)).all()
            worst = max(worst, float(np.abs(w32.astype(np.float64) - w64).max()))
    assert worst <= 2e-6, worst
