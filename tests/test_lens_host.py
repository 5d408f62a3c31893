"""CPU: the host side of the lens correction (pano360_amd/lens.py) - the focal length fit, the
calibration files, the command lines - and the conditions tests/lens_cases.py
must meet for tests/test_gpu_lens.py to mean what it says."""
import json

import numpy as np
import pytest

import lens_cases
import lens_model as lm
from pano360_amd import _lib, lens


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", lens_cases.CASES)
def test_cases_have_next_to_no_pixel_near_a_tie(name):
    """A condition on the cases, met by the model alone: the GPU test leaves out the pixels whose
    position is within 1e-6 of a 1/32 tie, and that exclusion must not be able to hide a failure."""
    for interp in lens_cases.INTERPS:
        want, near = lens_cases.expected(name, interp)
        w, h = lens_cases.CASES[name][6]
        assert want.shape == (h, w, 3) and near.shape == (h, w)
        assert near.sum() <= 1e-3 * near.size, (name, int(near.sum()))
        if name in lens_cases.FITTED:
            assert not near.any(), (name, int(near.sum()))


def test_model_identity_returns_the_input():
    img = lens_cases.image("identity")
    for interp in lens_cases.INTERPS:
        want, near = lens_cases.expected("identity", interp)
        assert np.array_equal(want, img) and not near.any()


def test_clamp_cases_leave_the_frame():
    """"clamp": positions pass the clamp to [-2, w + 1] x [-2, h + 1] on all four sides.  A
    fisheye of this focal length images the whole half space inside the frame's width, so
    "fisheye_clamp" leaves the frame only above and below."""
    kind, fx, fy, cx, cy, k, (w, h) = lens_cases.CASES["clamp"][:7]
    px, py = lm.position(kind, fx, fy, cx, cy, k, (w, h), lens_cases.focal("clamp"))
    assert px[:, 0].min() < -2 and px[:, -1].max() > w + 1
    assert py[0].min() < -2 and py[-1].max() > h + 1
    kind, fx, fy, cx, cy, k, (w, h) = lens_cases.CASES["fisheye_clamp"][:7]
    px, py = lm.position(kind, fx, fy, cx, cy, k, (w, h), lens_cases.focal("fisheye_clamp"))
    assert py[0].min() < -2 and py[-1].max() > h + 1


# ---------------------------------------------------------------- fit_focal
@pytest.mark.parametrize("name", lens_cases.FITTED + ("33x9",))
def test_fit_focal_keeps_every_pixel_inside(name):
    """At the returned focal length EVERY pixel of the output maps inside the source, not only the
    border (checked with the independent map of lens_model); at 0.999 x it some border pixel does
    not.

    The three stated values: the issue prints 97.763, 106.967 and 25.627 and asks for 1e-6
    relative, which three printed decimals cannot carry (97.763 alone is 5e-6 wide).  So the
    value must round to the printed one AND agree to 1e-6 relative with the bisection restated
    in lens_model on its own map (97.763185, 106.966537, 25.626992)."""
    kind, fx, fy, cx, cy, k, size = lens_cases.CASES[name][:7]
    model = lens_cases.lens_model(name)
    got = lens.fit_focal(model)
    assert got == lens.fit_focal(model, size)
    assert lm.inside(kind, fx, fy, cx, cy, k, size, got).all()
    assert not lm.inside(kind, fx, fy, cx, cy, k, size, 0.999 * got, border_only=True).all()
    want = lm.smallest_focal(kind, fx, fy, cx, cy, k, size)
    print(f"{name}: fit_focal {got!r}, model {want!r}")
    assert abs(got - want) <= 1e-6 * want
    if name in lens_cases.STATED_FOCALS:
        assert round(got, 3) == lens_cases.STATED_FOCALS[name]


def test_fit_focal_refusals():
    size = (131, 97)
    for cx, cy in ((-0.5, 48.0), (130.5, 48.0), (65.0, -1.0), (65.0, 96.5)):
        with pytest.raises(ValueError, match="principal point"):
            lens.fit_focal(lens.LensModel("brown", 100, 100, cx, cy, (), size))
    # a principal point on the frame's edge: what lies left of the centre maps outside at every
    # focal length, the bracket's upper end included
    with pytest.raises(ValueError, match="separates"):
        lens.fit_focal(lens.LensModel("brown", 100, 100, 0.0, 48.0, (), size))
    # 1 x 1: [0, w - 1] is the one point 0
    with pytest.raises(ValueError, match="principal point"):
        lens.fit_focal(lens_cases.lens_model("1x1"))
    with pytest.raises(ValueError, match="separates"):
        lens.fit_focal(lens.LensModel("brown", 10, 10, 0.0, 0.0, (0.1,), (1, 1)))


# ------------------------------------------------------------------- models
def test_lens_model_checks_its_arguments():
    m = lens.LensModel("brown", 100, 101, 60, 40, (0.1, 0.2), (120, 80))
    assert m.k == (0.1, 0.2, 0.0, 0.0, 0.0) and m.size == (120, 80)
    assert lens.LensModel("fisheye", 100, 101, 60, 40, (1, 2, 3, 4), (120, 80)).k == (1, 2, 3, 4, 0)
    for bad, what in ((dict(kind="equidistant"), "model"), (dict(k=(0,) * 6), "k"),
                      (dict(kind="fisheye", k=(0,) * 5), "k"), (dict(kind="fisheye", k=(0,) * 3), "k"),
                      (dict(fx=0.0), "fx"), (dict(fy=-1.0), "fy"), (dict(cx=float("nan")), "cx"),
                      (dict(k=(float("inf"),)), "k"), (dict(size=(0, 80)), "size"),
                      (dict(size=(120, 32768)), "size"), (dict(size=None), "size")):
        args = dict(kind="brown", fx=100.0, fy=101.0, cx=60.0, cy=40.0, k=(0.1,), size=(120, 80))
        args.update(bad)
        with pytest.raises(ValueError, match=what):
            lens.LensModel(**args)


def test_project_is_the_models_map():
    for name in ("barrel", "fisheye"):
        kind, fx, fy, cx, cy, k, size = lens_cases.CASES[name][:7]
        v, u = np.mgrid[0:size[1], 0:size[0]]
        px, py = lens_cases.lens_model(name).project(u, v, 77.0)
        qx, qy = lm.position(kind, fx, fy, cx, cy, k, size, 77.0)
        np.testing.assert_allclose(px, qx, rtol=0, atol=1e-9)
        np.testing.assert_allclose(py, qy, rtol=0, atol=1e-9)


def test_undistort_device_checks_before_it_needs_a_device():
    model = lens_cases.lens_model("barrel")
    frame = np.zeros((97, 131, 3), np.uint8)
    with pytest.raises(ValueError, match="131 x 97"):
        lens.undistort_device([np.zeros((97, 130, 3), np.uint8)], model)
    with pytest.raises(ValueError, match="2 models for 1 frames"):
        lens.undistort_device([frame], [model, model])
    with pytest.raises(ValueError, match="interp"):
        lens.undistort_device([frame], model, interp="nearest")
    with pytest.raises(ValueError, match="uint8"):
        lens.undistort_device([frame.astype(np.float32)], model)
    with pytest.raises(ValueError, match="2 focal lengths"):
        lens.undistort_device([frame], model, focal=[90.0, 91.0])
    assert lens.undistort_device([], model) == ([], [])


def test_rgb_on_device_copies_only_what_a_pitch_cannot_describe():
    """The frame helper of every stage (_lib.rgb_on_device), with the CPU standing in for the
    engine's device."""
    import types
    import warnings

    import torch
    eng = types.SimpleNamespace(device=torch.device("cpu"))
    rng = np.random.default_rng(7)
    pixels = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)

    def dense(t, w):
        return t.stride(2) == 1 and t.stride(1) == 3 and t.stride(0) >= 3 * w

    # a read-only array: copied, so that torch has nothing to warn about
    frozen = pixels.copy()
    frozen.setflags(write=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = _lib.rgb_on_device(frozen, eng)
    assert dense(got, 11) and np.array_equal(got.numpy(), pixels)
    assert not np.shares_memory(got.numpy(), frozen)
    # a strided array is made contiguous
    got = _lib.rgb_on_device(pixels[:, ::2], eng)
    assert dense(got, 6) and np.array_equal(got.numpy(), pixels[:, ::2])
    # the colour planes of an RGBA tensor: pixels 4 bytes apart, copied
    rgba = torch.from_numpy(rng.integers(0, 256, (9, 11, 4), dtype=np.uint8))
    view = rgba[..., :3]
    got = _lib.rgb_on_device(view, eng)
    assert got is not view and dense(got, 11) and torch.equal(got, view)
    assert got.data_ptr() != view.data_ptr()
    # a crop of a dense image: pixels 3 bytes apart, rows further: the same object
    image = torch.from_numpy(pixels.copy())
    crop = image[2:7, 3:9]
    assert crop.stride(0) > 3 * crop.shape[1] and not crop.is_contiguous()
    assert _lib.rgb_on_device(crop, eng) is crop
    assert _lib.rgb_on_device(image, eng) is image


# -------------------------------------------------------------------- files
ONE = {"model": "brown", "fx": 100.0, "fy": 101.0, "cx": 66.3, "cy": 47.1,
       "k": [-0.25, 0.05, 1e-3, -5e-4, 0.0], "size": [131, 97]}
FISH = {"model": "fisheye", "fx": 50.0, "fy": 50.0, "cx": 80.2, "cy": 59.7,
        "k": [0.02, -0.003, 0.0, 0.0], "size": [160, 120]}


def _write(tmp_path, record, name="lens.json"):
    path = tmp_path / name
    path.write_text(json.dumps(record))
    return str(path)


def test_load_both_file_shapes(tmp_path):
    cal = lens.load(_write(tmp_path, ONE))
    m = cal.model_for("anything.png")
    assert (m.kind, m.fx, m.fy, m.cx, m.cy, m.size) == ("brown", 100.0, 101.0, 66.3, 47.1, (131, 97))
    assert m.k == (-0.25, 0.05, 1e-3, -5e-4, 0.0) and cal.cameras == {} and cal.interp == "cubic"
    cal = lens.load(_write(tmp_path, {"default": ONE, "cameras": {"b.png": FISH}}))
    assert cal.model_for("a.png").kind == "brown"
    assert cal.model_for("b.png").kind == "fisheye" and cal.model_for("/some/dir/b.png").size == (160, 120)
    cal = lens.load(_write(tmp_path, {"cameras": {"b.png": FISH}}))
    assert cal.model_for("b.png").k == (0.02, -0.003, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="a.png"):
        cal.model_for("a.png")


def test_load_names_the_offending_key(tmp_path):
    for key in ONE:
        record = {k: v for k, v in ONE.items() if k != key}
        with pytest.raises(ValueError, match=f"missing key '{key}'"):
            lens.load(_write(tmp_path, record))
    with pytest.raises(ValueError, match="unknown key 'k4'"):
        lens.load(_write(tmp_path, dict(ONE, k4=0.0)))
    with pytest.raises(ValueError, match="unknown key 'rig'"):
        lens.load(_write(tmp_path, {"default": ONE, "rig": 1}))
    with pytest.raises(ValueError, match="'cameras': 'b.png'.*missing key 'fy'"):
        lens.load(_write(tmp_path, {"cameras": {"b.png": {k: v for k, v in FISH.items() if k != "fy"}}}))
    with pytest.raises(ValueError, match="'default'.*unknown key 'p1'"):
        lens.load(_write(tmp_path, {"default": dict(ONE, p1=0.0)}))
    # a wrong coefficient count, an unknown model
    with pytest.raises(ValueError, match="k: 6 coefficients"):
        lens.load(_write(tmp_path, dict(ONE, k=[0.0] * 6)))
    with pytest.raises(ValueError, match="k: 5 coefficients"):
        lens.load(_write(tmp_path, dict(FISH, k=[0.0] * 5)))
    with pytest.raises(ValueError, match="model 'thin_prism'"):
        lens.load(_write(tmp_path, dict(ONE, model="thin_prism")))
    with pytest.raises(ValueError, match="without a model"):
        lens.load(_write(tmp_path, {"cameras": {}}))


# ------------------------------------------------------------- command lines
OLD_STITCHER_DEFAULTS = dict(
    path="DIR", shrink=2, ba="incr", equalize=False, crop=False, blend="multiband", ghost_tol=None,
    out=None, register=False, detector="sift", view=[], equirect=None, cube=None, deepzoom=False,
    multires=None, tile=512, fill=False)


def test_stitcher_command_line():
    import stitcher
    args = stitcher.parse_args(["DIR"])
    assert vars(args) == dict(OLD_STITCHER_DEFAULTS, lens=None, lens_interp=None, lens_focal=None)
    assert stitcher.cache_name(args) == "DIR_s2"
    assert stitcher.cache_name(stitcher.parse_args(["some/DIR/", "-s", "1.5", "--detector", "msop"])) \
        == "DIR_s1.5_msop"
    args = stitcher.parse_args(["DIR", "--lens", "rig.json"])
    assert (args.lens, args.lens_interp, args.lens_focal) == ("rig.json", None, None)
    assert stitcher.cache_name(args) == "DIR_s2_lens"
    args = stitcher.parse_args(["DIR", "--lens", "rig.json", "--detector", "msop", "--lens-interp",
                                "linear", "--lens-focal", "812.5"])
    assert stitcher.cache_name(args) == "DIR_s2_msop_lens"
    assert (args.lens_interp, args.lens_focal) == ("linear", 812.5)
    for bad in (["--lens-interp", "cubic"], ["--lens-focal", "800"],
                ["--lens", "rig.json", "--lens-interp", "nearest"],
                ["--lens", "rig.json", "--lens-focal", "0"],
                ["--lens", "rig.json", "--lens-focal", "nan"]):
        with pytest.raises(SystemExit) as err:
            stitcher.parse_args(["DIR"] + bad)
        assert err.value.code == 2, bad


def test_features_command_line():
    from pano360_amd import features
    args = features.parse_args(["--path", "some/DIR"])
    assert vars(args) == dict(path="some/DIR", detector="sift", lens=None, lens_interp=None,
                              lens_focal=None)
    assert features.cache_name(args) == "DIR"
    assert features.cache_name(features.parse_args(["--path", "DIR", "--detector", "msop"])) == "DIR_msop"
    assert features.cache_name(features.parse_args(["--path", "DIR", "--lens", "l.json"])) == "DIR_lens"
    assert features.cache_name(features.parse_args(["--path", "DIR", "--lens", "l.json", "--detector",
                                                    "msop"])) == "DIR_msop_lens"
    for bad in (["--lens-interp", "linear"], ["--lens-focal", "800"]):
        with pytest.raises(SystemExit) as err:
            features.parse_args(["--path", "DIR"] + bad)
        assert err.value.code == 2, bad


def test_from_args_resolves_the_defaults(tmp_path):
    import stitcher
    path = _write(tmp_path, ONE)
    assert lens.from_args(stitcher.parse_args(["DIR"])) is None
    cal = lens.from_args(stitcher.parse_args(["DIR", "--lens", path]))
    assert (cal.interp, cal.focal) == ("cubic", None)
    cal = lens.from_args(stitcher.parse_args(["DIR", "--lens", path, "--lens-interp", "linear",
                                              "--lens-focal", "90"]))
    assert (cal.interp, cal.focal) == ("linear", 90.0)


def test_top_level_module_re_exports():
    import lens as top
    for name in ("LensModel", "load", "fit_focal", "undistort_device", "undistort"):
        assert getattr(top, name) is getattr(lens, name)

