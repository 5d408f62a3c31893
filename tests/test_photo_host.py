"""CPU: the host side of the photometric alignment (pano360_amd/photo.py) - the solve, the pair
table, the lattice step, the argument checks, the command line and the binding - against the NumPy
statement (tests/photo_model.py) on the forged rigs of tests/photo_cases.py.

The caps: 0.005 in a log-gain and in log V anywhere on a frame, about one 8-bit level at 200.
They are the issue's; the scenes were made to fit them (tests/photo_cases.py says how the
walker's rectangles were sized), not the other way round."""
import logging

import numpy as np
import pytest

import photo_cases as pc
import photo_model as pm
from pano360_amd import _lib, photo

CAP = 0.005
TAU = 0.05


def _fit(name, rounds, step=1, terms=2):
    """``photo.solve`` driven by the model's sums: the passes of ``estimate_device``."""
    frames, pairs = pc.frames(name), list(pc.pairs(name))
    model = photo.solve(len(frames), pairs, pc.first_pass(name, step)[0], terms)
    for _ in range(rounds):
        sums, _ = pm.stats(frames, pairs, pc.LO, pc.HI, step, model.log_gains, model.alpha, TAU)
        model = photo.solve(len(frames), pairs, sums, terms)
    return model


# ------------------------------------------------------------------- the solve
@pytest.mark.parametrize("step", pc.STEPS)
@pytest.mark.parametrize("name", pc.RECOVERABLE)
def test_solve_recovers_the_truth(name, step):
    model = _fit(name, photo.ROUNDS, step)
    d_gain, d_fall = pc.errors(name, model.log_gains, model.alpha)
    print(f"{name} step {step}: max |d log-gain| {d_gain:.5f}, max |d log V| {d_fall:.5f}, "
          f"rms {model.rms:.5f}, weight {model.weight:.1f}")
    assert d_gain <= CAP and d_fall <= CAP
    assert np.abs(model.log_gains.mean(axis=0)).max() < 1e-12
    assert model.alpha[2] == 0.0
    # ... and it is the model's own solve of the same sums
    lg, alpha, _ = pc.estimate(name, photo.ROUNDS, step)
    assert np.abs(model.log_gains - lg).max() < 1e-9 and np.abs(model.alpha - alpha).max() < 1e-9


def test_the_passes_matter():
    """Without reweighting the walker's rectangles pull the fit past the cap."""
    model = _fit("walker", 0)
    d_gain, d_fall = pc.errors("walker", model.log_gains, model.alpha)
    print(f"walker, first pass alone: {d_gain:.5f}, {d_fall:.5f}")
    assert d_gain > CAP and d_fall > CAP


def test_gains_alone_leave_the_falloff_in():
    """``terms = 0`` on vignetted frames: the gains still come out (to what the falloff leaks
    into them), alpha stays zero, and the corrected overlaps differ more than with the falloff."""
    name = "rig5"
    frames, pairs = pc.frames(name), list(pc.pairs(name))
    flat = _fit(name, photo.ROUNDS, terms=0)
    assert not flat.alpha.any()
    full = _fit(name, photo.ROUNDS)
    assert flat.rms > 2 * full.rms

    def after(model):
        fixed = [pm.apply(f, pm.table(lg, model.alpha)) for f, lg in zip(frames, model.log_gains)]
        return pm.overlap_difference(fixed, pairs)
    assert after(flat) > 2 * after(full)


@pytest.mark.parametrize("name", ("rig5", "rig3", "mixed", "behind", "flat"))
def test_corrected_overlaps_agree(name):
    frames, pairs = pc.frames(name), list(pc.pairs(name))
    model = _fit(name, photo.ROUNDS)
    tables = photo.tables(model)
    assert tables.shape == (len(frames), 3, pm.TABLE) and tables.dtype == np.float32
    for k, lg in enumerate(model.log_gains):
        assert np.array_equal(tables[k], pm.table(lg, model.alpha))
    fixed = [pm.apply(f, t) for f, t in zip(frames, tables)]
    before = pm.overlap_difference(frames, pairs)
    after = pm.overlap_difference(fixed, pairs)
    clean = pm.overlap_difference(pc.clean_frames(name), pairs)
    print(f"{name}: mean overlap difference {before:.2f} -> {after:.2f} levels (clean {clean:.2f})")
    assert after <= clean + 0.5 and after <= before / 4


def test_solve_edge_cases(caplog):
    pairs = [(0, 1, np.eye(3))]
    with caplog.at_level(logging.WARNING):
        model = photo.solve(3, [], np.zeros((0, 25)))
    assert "no camera pair" in caplog.text
    assert not model.log_gains.any() and model.log_gains.shape == (3, 3) and not model.alpha.any()
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        model = photo.solve(2, pairs, np.zeros((1, 25)))           # a pair without a sample
    assert "no camera pair" in caplog.text and not model.log_gains.any()
    # samples whose e_k all vanish do not determine a falloff term
    sums = np.zeros((1, 25))
    sums[0, 0] = 100.0
    sums[0, 10], sums[0, 15], sums[0, 20] = 10.0, 20.0, -10.0
    sums[0, 14], sums[0, 19], sums[0, 24] = 1.0, 4.0, 1.0
    with pytest.raises(ValueError, match="singular"):
        photo.solve(2, pairs, sums, terms=2)
    model = photo.solve(2, pairs, sums, terms=0)
    # d = lg0 - lg1 = 0.1, 0.2, -0.1 per channel, shrunk by the ridge by a part in 1e4 or so
    assert np.allclose(model.log_gains[0] - model.log_gains[1], [0.1, 0.2, -0.1], rtol=1e-3)
    assert np.allclose(model.log_gains[0], -model.log_gains[1])
    for bad in (dict(n=0), dict(terms=4), dict(terms=-1), dict(prior=0.0), dict(sums=np.zeros((2, 25))),
                dict(sums=np.full((1, 25), np.nan))):
        args = dict(dict(n=2, pairs=pairs, sums=sums, terms=0, prior=1e-4), **bad)
        with pytest.raises(ValueError):
            photo.solve(**args)


# ------------------------------------------------------------------- the pairs
@pytest.mark.parametrize("name", pc.CASES)
def test_pair_table_keeps_every_pair_with_a_sample(name):
    rots, intrs = pc.cameras(name)
    frames = pc.frames(name)
    table = photo.pair_table([f.shape[:2] for f in frames], rots, intrs)
    listed = {(i, j): H for i, j, H in table}
    assert all(i < j for i, j in listed) and len(listed) == len(table)
    for i, j, H in pc.pairs(name):
        # (any sample at all: the range test left out)
        hit = len(pm.samples(frames[i], frames[j], H, 0, 255, 1)[0])
        assert not hit or (i, j) in listed, (i, j, hit)
        if (i, j) in listed:
            assert np.allclose(listed[(i, j)], H, rtol=1e-12, atol=1e-12)
    if name == "apart":
        assert table == []
    if name == "behind":
        assert len(table) < len(pc.pairs(name))


def test_pair_table_of_a_long_ring_is_short():
    from pano360_amd import synth
    rots, intrs = synth.make_cameras(120, 7680, 4320, step_deg=3.0)
    table = photo.pair_table([(4320, 7680)] * 120, rots, intrs)
    # hfov 60 degrees, 3 degrees a camera: a camera can share a ray with about 23 on either side
    assert 120 * 19 < len(table) < 120 * 28 < 7140
    assert {(i, i + 1) for i in range(119)} <= {(i, j) for i, j, _ in table}
    with pytest.raises(ValueError):
        photo.pair_table([(4, 4)] * 2, rots[:3], intrs[:2])


def test_default_step():
    assert photo.default_step([(2160, 3840)]) == 6
    assert photo.default_step([(1080, 1920)]) == 3
    assert photo.default_step([(511, 511)]) == photo.default_step([(512, 512)]) == 1
    assert photo.default_step([(512, 513)]) == 2
    assert photo.default_step([(64, 96), (2160, 3840), (40, 48)]) == 6
    assert photo.default_step([]) == 1
    for shape in ((2160, 3840), (4320, 7680), (1000, 3000)):
        step = photo.default_step([shape])
        assert -(-shape[0] // step) * -(-shape[1] // step) <= 1 << 18
        assert -(-shape[0] // (step - 1)) * -(-shape[1] // (step - 1)) > 1 << 18


# ------------------------------------------------------------- argument errors
def test_argument_errors_come_before_the_device():
    """(none of these reaches the engine: they pass without a GPU)"""
    frame = np.zeros((4, 6, 3), np.uint8)
    eye = [np.eye(3)] * 2
    for bad in (dict(step=0), dict(step=40000), dict(lo=0), dict(hi=256), dict(lo=200, hi=100),
                dict(tau=0.0), dict(tau=float("nan")), dict(rots=eye[:1]),
                dict(params=photo.PhotoModel(np.zeros((3, 3)))),
                dict(params=photo.PhotoModel(np.full((2, 3), np.inf)))):
        args = dict(dict(frames=[frame, frame], rots=eye, intrs=eye, lo=16, hi=239, step=1), **bad)
        with pytest.raises(ValueError):
            photo.stats_device(**args)
    with pytest.raises(ValueError):
        photo.apply_device([frame], photo.PhotoModel(np.zeros((2, 3))))
    with pytest.raises(ValueError):
        photo.estimate_device([frame, frame], eye, eye, rounds=-1)
    assert photo.apply_device([], photo.PhotoModel(np.zeros((0, 3)))) == []


# ---------------------------------------------------------------- command line
def test_command_line():
    import stitcher
    args = stitcher.parse_args(["DIR"])
    assert photo.mode_of(args) is None and "photometric" not in vars(args)    # the namespace it was
    for mode, terms in (("color", 0), ("vignette", 2)):
        chosen = stitcher.parse_args(["DIR", "--photometric", mode, "-b", "median", "--crop"])
        assert photo.mode_of(chosen) == chosen.photometric == mode and photo.MODES[mode] == terms
        # registration sees the frames as they were: no cache name changes
        assert stitcher.cache_name(chosen) == stitcher.cache_name(args) == "DIR_s2"
    for bad in (["--photometric", "vignette", "--equalize"], ["--photometric", "color", "-e"],
                ["--photometric", "gamma"], ["--photometric"]):
        with pytest.raises(SystemExit) as err:
            stitcher.parse_args(["DIR"] + bad)
        assert err.value.code == 2, bad


def test_top_level_module_re_exports():
    import photo as top
    for name in ("PhotoModel", "pair_table", "stats_device", "default_step", "solve",
                 "estimate_device", "apply_device", "correct_regions"):
        assert getattr(top, name) is getattr(photo, name)


# ---------------------------------------------------------------------- ABI
def test_constants_are_the_models():
    assert [_lib.PHOTO_MAX_SIDE, _lib.PHOTO_SUMS, _lib.PHOTO_TABLE] == [32767, 25, 1026]
    assert photo.SUMS == pm.SUMS and photo.TABLE == pm.TABLE
