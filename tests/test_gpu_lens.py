"""GPU: the lens correction (pano360_amd/lens.py, csrc/lens.hip) against its NumPy statement
(tests/lens_model.py) and against exact properties.

A pixel must equal the model's unless its sampling position lies within 1e-6 of a 1/32 tie
(``lens_model.near_tie``): the device and NumPy evaluate the same float64 operations, only ``atan``
may differ by a few units in the last place, so the two values of 32 p differ by less than 1e-9
and the quantisation can only differ inside a band a thousandth as wide as the one left out.
tests/test_lens_host.py shows that at most 0.1 % of a case's pixels, and none of a Brown case's,
lie in the band.  How many were left out and how many of those differ is printed, not asserted.
Everything else here is exact: equalities between device results."""
import ctypes as C
import json
import os
import pickle

import numpy as np
import pytest
import torch

import lens_cases
from pano360_amd import _lib, lens

pytestmark = pytest.mark.gpu


def _correct(eng, name, interp):
    outs, focals = lens.undistort([lens_cases.image(name)], lens_cases.lens_model(name), interp,
                                  lens_cases.focal(name), eng)
    assert focals == [lens_cases.focal(name)]
    return outs[0]


# --------------------------------------------------------------- against the model
@pytest.mark.parametrize("interp", lens_cases.INTERPS)
@pytest.mark.parametrize("name", lens_cases.CASES)
def test_undistort_equals_the_model(eng, name, interp):
    want, near = lens_cases.expected(name, interp)
    got = _correct(eng, name, interp)
    assert got.shape == want.shape and got.dtype == np.uint8
    differ = (got != want).any(axis=-1)
    print(f"{name} {interp}: {near.size} pixels, {int(near.sum())} near a tie left out, "
          f"{int((differ & near).sum())} of those differ from the model")
    if lens_cases.CASES[name][0] == "brown":
        assert not near.any()
    assert not differ[~near].any(), (name, interp, int(differ[~near].sum()))
    assert np.array_equal(_correct(eng, name, interp), got)        # the same bytes on a second call


@pytest.mark.parametrize("interp", lens_cases.INTERPS)
def test_identity_returns_the_input(eng, interp):
    assert np.array_equal(_correct(eng, "identity", interp), lens_cases.image("identity"))


def test_fitted_focal_is_the_default(eng):
    names = list(lens_cases.FITTED)
    frames = [torch.from_numpy(lens_cases.image(n).copy()).to(eng.device) for n in names]
    models = [lens_cases.lens_model(n) for n in names]
    outs, focals = lens.undistort_device(frames, models, eng=eng)
    assert focals == [lens.fit_focal(m) for m in models]
    again, same = lens.undistort_device(frames, models, "cubic", focals, eng)
    assert same == focals and all(torch.equal(a, b) for a, b in zip(outs, again))
    # a list with a hole: that frame's focal length is fitted
    mixed, got = lens.undistort_device(frames, models, focal=[focals[0], None, focals[2]], eng=eng)
    assert got == focals and all(torch.equal(a, b) for a, b in zip(outs, mixed))


# ----------------------------------------------------------------------- batches
BATCH = ("barrel", "1x1", "fisheye_clamp", "33x9", "4wide")


@pytest.mark.parametrize("interp", lens_cases.INTERPS)
def test_a_batch_equals_single_calls(eng, interp):
    """Five frames of different sizes and models, with and without borders that clamp, in one call."""
    frames = [torch.from_numpy(lens_cases.image(n).copy()).to(eng.device) for n in BATCH]
    models = [lens_cases.lens_model(n) for n in BATCH]
    focals = [lens_cases.focal(n) for n in BATCH]
    outs, got = lens.undistort_device(frames, models, interp, focals, eng)
    assert got == focals and len(outs) == len(BATCH)
    for name, frame, model, focal, out in zip(BATCH, frames, models, focals, outs):
        single, _ = lens.undistort_device([frame], model, interp, focal, eng)
        assert torch.equal(out, single[0]), name
        assert tuple(out.shape) == tuple(frame.shape) and out.is_contiguous()


def test_more_frames_than_one_launch_takes(eng):
    """The call takes any number of frames: 64 go into a launch, here 131 small ones."""
    names = ["33x9", "1x1", "4wide"] * 43 + ["33x9", "1x1"]
    frames = [torch.from_numpy(lens_cases.image(n).copy()).to(eng.device) for n in names]
    outs, _ = lens.undistort_device(frames, [lens_cases.lens_model(n) for n in names], "cubic",
                                    [lens_cases.focal(n) for n in names], eng)
    want = {n: _correct(eng, n, "cubic") for n in set(names)}
    for name, out in zip(names, outs):
        assert np.array_equal(out.cpu().numpy(), want[name]), name


# ----------------------------------------------------------------------- pitches
@pytest.mark.parametrize("interp", lens_cases.INTERPS)
def test_pitched_source_and_destination(eng, interp):
    """A source that is a rectangle of a larger tensor (pitch > 3 w, its base and rows at any
    alignment) gives the contiguous result and stays as it is; a pitched destination's bytes beyond
    the frame are untouched (through the C ABI: ``undistort_device`` allocates its outputs)."""
    name = "barrel"
    img, model, focal = lens_cases.image(name), lens_cases.lens_model(name), lens_cases.focal(name)
    h, w = img.shape[:2]
    want = _correct(eng, name, interp)
    big = lens_cases.noise(h + 9, w + 14, 3)
    big[4:4 + h, 5:5 + w] = img
    dev = torch.from_numpy(big).to(eng.device)
    view = dev[4:4 + h, 5:5 + w]
    assert view.stride(0) > 3 * w and view.data_ptr() % 4 != 0
    outs, _ = lens.undistort_device([view], model, interp, focal, eng)
    assert np.array_equal(outs[0].cpu().numpy(), want)
    assert np.array_equal(dev.cpu().numpy(), big)
    for x0, extra in ((2, 7), (4, 4)):                  # rows off and on four bytes
        target = torch.full((h + 3, w + extra, 3), 77, dtype=torch.uint8, device=eng.device)
        inner = target[1:1 + h, x0:x0 + w]
        rec = _lib.LensFrame(view.data_ptr(), inner.data_ptr(), view.stride(0), inner.stride(0),
                             model.fx, model.fy, model.cx, model.cy, focal,
                             (C.c_double * 5)(*model.k), w, h, lens.KINDS[model.kind],
                             lens.INTERPS[interp])
        _lib.check(eng.lib.pano_lens_undistort_u8(eng.ctx(), C.byref(rec), 1), "pano_lens_undistort_u8")
        host = target.cpu().numpy()
        assert np.array_equal(host[1:1 + h, x0:x0 + w], want)
        host[1:1 + h, x0:x0 + w] = 77
        assert (host == 77).all()
    # a tensor whose pixels are not contiguous is copied first
    rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device=eng.device)
    rgba[..., :3] = torch.from_numpy(img.copy()).to(eng.device)
    assert rgba[..., :3].stride(1) == 4
    outs, _ = lens.undistort_device([rgba[..., :3]], model, interp, focal, eng)
    assert np.array_equal(outs[0].cpu().numpy(), want)


# ------------------------------------------------------------------- error paths
def test_the_abi_refuses_bad_arguments(eng):
    src = torch.full((6, 8, 3), 9, dtype=torch.uint8, device=eng.device)
    dst = torch.full((6, 8, 3), 77, dtype=torch.uint8, device=eng.device)
    good = dict(src=src.data_ptr(), dst=dst.data_ptr(), src_pitch=24, dst_pitch=24, fx=10.0, fy=10.0,
                cx=4.0, cy=3.0, f_new=10.0, k=(0.1, 0.0, 0.0, 0.0, 0.0), w=8, h=6, model=0, interp=0)

    def call(n=1, null=False, **change):
        fields = dict(good, **change)
        fields["k"] = (C.c_double * 5)(*fields["k"])
        recs = (_lib.LensFrame * 2)(_lib.LensFrame(**dict(good, k=(C.c_double * 5)(*good["k"]))),
                                    _lib.LensFrame(**fields))
        return eng.lib.pano_lens_undistort_u8(eng.ctx(), None if null else recs, n + 1 if n else 0)
    inf, nan = float("inf"), float("nan")
    for bad in (dict(n=0), dict(n=-2), dict(null=True), dict(src=None), dict(dst=None),
                dict(w=0), dict(h=0), dict(w=32768), dict(h=32768), dict(src_pitch=23),
                dict(dst_pitch=23), dict(dst=src.data_ptr()), dict(dst=src.data_ptr() + 24 * 5 + 23),
                dict(src=dst.data_ptr() + 3), dict(k=(0.0, nan, 0.0, 0.0, 0.0)),
                dict(k=(0.0, 0.0, 0.0, 0.0, inf)), dict(fx=nan), dict(cy=inf), dict(f_new=inf),
                dict(fx=0.0), dict(fy=-1.0), dict(f_new=0.0), dict(model=2), dict(model=-1),
                dict(interp=2)):
        assert call(**bad) == _lib.EINVAL, bad
        assert b"pano_lens_undistort_u8" in eng.lib.pano_last_error()
    torch.cuda.synchronize()
    assert int(dst.min()) == 77 == int(dst.max())       # nothing was launched, the good record neither
    # neighbours that do not overlap are taken
    both = torch.zeros((12, 8, 3), dtype=torch.uint8, device=eng.device)
    assert call(src=both.data_ptr(), dst=both.data_ptr() + 6 * 24) == 0
    assert call(src=both.data_ptr() + 6 * 24, dst=both.data_ptr()) == 0
    torch.cuda.synchronize()
    # the Python layer refuses a frame that is not its calibration's size, before anything runs
    with pytest.raises(ValueError, match="131 x 97"):
        lens.undistort_device([src], lens_cases.lens_model("barrel"), eng=eng)


# -------------------------------------------------------------------- end to end
def test_cli_lens(eng, tmp_path, monkeypatch):
    import bundle_adj
    import stitcher as top
    from PIL import Image
    from pano360_amd import synth
    imgs, rots, intrs = synth.make_scene(4, 200, 120, sweep_deg=60.0, jitter=0.01, seed=5, kind="B")
    rig = tmp_path / "RIG"
    rig.mkdir()
    for i, im in enumerate(imgs):
        Image.fromarray(np.ascontiguousarray(im[..., ::-1])).save(rig / f"frame{i}.png")
    files = [f for f in os.listdir(rig) if f.endswith(".png")]
    order = [int(f[5:-4]) for f in files]               # the ingest reads in os.listdir order

    def cameras():
        return [bundle_adj.Image(None, rots[i], intrs[i]) for i in order]
    for cache in ("ba_RIG_s1.0_lens.pkl", "ba_RIG_s1.0.pkl"):
        with open(tmp_path / cache, "wb") as fid:
            pickle.dump(cameras(), fid, protocol=pickle.HIGHEST_PROTOCOL)
    one = {"model": "brown", "fx": 150.0, "fy": 151.0, "cx": 101.2, "cy": 58.9,
           "k": [-0.2, 0.04, 1e-3, -5e-4, 0.0], "size": [200, 120]}
    other = dict(one, k=[0.1], cx=99.0)
    (tmp_path / "lens.json").write_text(json.dumps({"default": one, "cameras": {"frame2.png": other}}))
    monkeypatch.chdir(tmp_path)

    raw = top.ingest(str(rig), 1)
    assert [tuple(f.shape) for f in raw] == [(120, 200, 3)] * 4
    for i, frame in zip(order, raw):
        assert np.array_equal(frame.cpu().numpy(), imgs[i])         # lossless, BGR
    cal = lens.load(str(tmp_path / "lens.json"))
    models = [cal.model_for(f) for f in files]
    assert [m.k[0] for m in models] == [0.1 if f == "frame2.png" else -0.2 for f in files]
    for interp in ("cubic", "linear"):
        flags = [] if interp == "cubic" else ["--lens-interp", "linear"]
        got = top.main([str(rig), "--lens", "lens.json", "-b", "linear", "-s", "1"] + flags)
        corrected, focals = lens.undistort_device(raw, models, interp, eng=eng)
        assert all(not torch.equal(a, b) for a, b in zip(corrected, raw))
        regions = cameras()
        for reg, frame in zip(regions, corrected):
            reg.img = frame
        want = top.stitch(regions, blender=top.linear_blend)
        assert np.array_equal(got, want), interp
    # an override of the focal length reaches the kernel
    got = top.main([str(rig), "--lens", "lens.json", "-b", "linear", "-s", "1", "--lens-focal", "170"])
    corrected, focals = lens.undistort_device(raw, models, focal=170.0, eng=eng)
    regions = cameras()
    for reg, frame in zip(regions, corrected):
        reg.img = frame
    assert focals == [170.0] * 4 and np.array_equal(got, top.stitch(regions, blender=top.linear_blend))
    # with a shrink the correction comes first, at the files' resolution
    with open(tmp_path / "ba_RIG_s2.0_lens.pkl", "wb") as fid:
        pickle.dump(cameras(), fid, protocol=pickle.HIGHEST_PROTOCOL)
    shrunk = top.ingest(str(rig), 2.0, lens=cal)
    corrected, _ = lens.undistort_device(raw, models, eng=eng)
    from pano360_amd import blend
    for a, b in zip(shrunk, corrected):
        assert torch.equal(a, blend.shrink_device(b, 2.0, eng))
    assert all(torch.equal(a, b) for a, b in zip(top.ingest(str(rig), 1, decode="host", lens=cal), corrected))
    # without --lens: its own cache, and what it returned before - the stitch of the raw frames
    plain = top.main([str(rig), "-b", "linear", "-s", "1"])
    regions = cameras()
    for reg, frame in zip(regions, raw):
        reg.img = frame
    assert np.array_equal(plain, top.stitch(regions, blender=top.linear_blend))
    assert plain.shape != want.shape or not np.array_equal(plain, want)
