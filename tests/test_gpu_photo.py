"""GPU: the photometric alignment (pano360_amd/photo.py, csrc/photo.hip) against its NumPy
statement (tests/photo_model.py) on the forged rigs of tests/photo_cases.py, and against exact
properties.

The statistics: the device and the model take the same samples - positions, taps and the range
test use exactly rounded operations only -, so with every weight 1 the count must be EQUAL.  Every
other sum may differ by the order of its additions and by ``log`` (a few units in the last place):
|device - model| <= 1e-9 A + 1e-12 sum(w), A the sum of the absolute values of that sum's terms
(the model returns it).  float64 with at most 1e6 additions in any order bounds the difference by
1.1e-10 A.  The correction is compared on every pixel.  Everything else is an equality between
device results."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest
import torch

import photo_cases as pc
import photo_model as pm
from pano360_amd import _lib, photo

pytestmark = pytest.mark.gpu

CAP = 0.005
TAU = 0.05


def _close(got, want, scale):
    count = want[:, :1]
    return np.abs(got - want) <= 1e-9 * scale + 1e-12 * count


def _device_stats(eng, name, step, params=None, tau=np.inf, pairs=None):
    rots, intrs = pc.cameras(name)
    pairs = list(pc.pairs(name)) if pairs is None else pairs
    listed, sums = photo.stats_device(pc.frames(name), rots, intrs, pc.LO, pc.HI, step, params, tau,
                                      eng, pairs)
    assert [(i, j) for i, j, _ in listed] == [(i, j) for i, j, _ in pairs]
    assert sums.shape == (len(pairs), pm.SUMS) and sums.dtype == np.float64
    return sums


# ------------------------------------------------------------- the statistics
@pytest.mark.parametrize("step", pc.STEPS)
@pytest.mark.parametrize("name", pc.CASES)
def test_stats_equal_the_model(eng, name, step):
    want, scale = pc.first_pass(name, step)
    got = _device_stats(eng, name, step)
    assert np.isfinite(got).all()
    worst = np.max(np.abs(got - want) / np.maximum(scale, 1e-300), initial=0.0)
    print(f"{name} step {step}: counts {[int(c) for c in got[:, 0]]}, "
          f"max |device - model| / A = {worst:.2e}")
    assert np.array_equal(got[:, 0], want[:, 0])                    # the same samples
    assert _close(got, want, scale).all()
    # a pair without a sample is 25 zeros, exactly
    empty = want[:, 0] == 0
    assert not got[empty].any() and not np.signbit(got[empty]).any()
    if name in ("apart", "clipped", "behind"):
        assert empty.any()
    if name == "apart":
        assert empty.all()
    if name == "clipped":
        clip = pc.CASES[name]["clip"]
        assert all(empty[k] for k, (i, j, _) in enumerate(pc.pairs(name)) if clip in (i, j))
    # the same bytes on a second call
    assert np.array_equal(_device_stats(eng, name, step).view(np.uint64), got.view(np.uint64))


@pytest.mark.parametrize("step", pc.STEPS)
@pytest.mark.parametrize("name", pc.CASES)
def test_reweighted_stats_equal_the_model(eng, name, step):
    """A pass with the model's first-pass parameters and tau = 0.05."""
    want, scale = pc.second_pass(name, step)
    lg, alpha = pc.first_params(name, step)
    got = _device_stats(eng, name, step, photo.PhotoModel(lg, alpha), TAU)
    assert np.isfinite(got).all()
    first = pc.first_pass(name, step)[0]
    worst = np.max(np.abs(got - want) / np.maximum(scale, 1e-300), initial=0.0)
    print(f"{name} step {step}: weight {got[:, 0].sum():.2f} of {first[:, 0].sum():.0f} samples, "
          f"max |device - model| / A = {worst:.2e}")
    assert _close(got, want, scale).all()
    assert (got[:, 0] <= first[:, 0]).all()
    if name == "walker":
        assert got[:, 0].sum() < first[:, 0].sum() - 100          # the rectangles lost their weight
    assert not got[want[:, 0] == 0].any()


def test_a_batch_equals_single_calls(eng):
    """A pair's sums do not depend on what else is in the batch: mixed sizes, empty pairs, more
    pairs than one launch takes."""
    for name, step in (("mixed", 1), ("behind", 3)):
        pairs = list(pc.pairs(name))
        lg, alpha = pc.first_params(name, step)
        for params, tau in ((None, np.inf), (photo.PhotoModel(lg, alpha), TAU)):
            batch = _device_stats(eng, name, step, params, tau)
            for k, pair in enumerate(pairs):
                single = _device_stats(eng, name, step, params, tau, [pair])
                assert np.array_equal(single[0].view(np.uint64), batch[k].view(np.uint64)), (name, k)
            # ... nor on its place in it
            back = _device_stats(eng, name, step, params, tau, pairs[::-1])
            assert np.array_equal(back[::-1].view(np.uint64), batch.view(np.uint64))
            # ... nor on the launch that takes it: the twelve ordered pairs, 22 times over, are 264
            # pairs, more than one launch's 256; the second launch's table and partials continue
            # where the first one's end
            if name == "mixed":
                ordered = pairs + [(j, i, np.linalg.inv(H)) for i, j, H in pairs]
                twelve = _device_stats(eng, name, step, params, tau, ordered)
                assert len(twelve) == 12
                assert np.array_equal(twelve[:6].view(np.uint64), batch.view(np.uint64))
                many = _device_stats(eng, name, step, params, tau, ordered * 22)
                assert len(many) == 264
                for k in range(len(many)):
                    assert np.array_equal(many[k].view(np.uint64), twelve[k % 12].view(np.uint64)), k


def test_stats_take_pitched_device_frames_and_the_default_pairs(eng):
    name = "rig5"
    rots, intrs = pc.cameras(name)
    frames = pc.frames(name)
    h, w = frames[0].shape[:2]
    views = []
    for k, frame in enumerate(frames):
        big = torch.full((h + 5, w + 7, 3), 255, dtype=torch.uint8, device=eng.device)
        view = big[2:2 + h, 3 + k % 2:3 + k % 2 + w]
        view.copy_(torch.from_numpy(frame.copy()).to(eng.device))
        assert view.stride(0) > 3 * w
        views.append(view)
    want = _device_stats(eng, name, 1)
    _, got = photo.stats_device(views, rots, intrs, pc.LO, pc.HI, 1, eng=eng, pairs=list(pc.pairs(name)))
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # pair_table's own list: the pairs that can overlap, the same samples
    listed, sums = photo.stats_device(views, rots, intrs, pc.LO, pc.HI, 1, eng=eng)
    index = {(i, j): k for k, (i, j, _) in enumerate(pc.pairs(name))}
    assert {(i, j) for (i, j), k in index.items() if want[k, 0] > 0} <= {(i, j) for i, j, _ in listed}
    for (i, j, _), row in zip(listed, sums):
        assert row[0] == want[index[(i, j)], 0]


# ------------------------------------------------------------------- the fit
@pytest.mark.parametrize("name", pc.RECOVERABLE)
def test_estimate_recovers_the_truth(eng, name):
    rots, intrs = pc.cameras(name)
    model = photo.estimate_device(pc.frames(name), rots, intrs, terms=2, eng=eng)
    d_gain, d_fall = pc.errors(name, model.log_gains, model.alpha)
    lg, alpha, _ = pc.estimate(name)
    print(f"{name}: max |d log-gain| {d_gain:.5f}, max |d log V| {d_fall:.5f}; against the model's "
          f"own estimate {np.abs(model.log_gains - lg).max():.2e}, {np.abs(model.alpha - alpha).max():.2e}")
    assert d_gain <= CAP and d_fall <= CAP
    if name == "walker":
        alone = photo.estimate_device(pc.frames(name), rots, intrs, terms=2, rounds=0, eng=eng)
        assert max(pc.errors(name, alone.log_gains, alone.alpha)) > CAP
    if name == "flat":
        colour = photo.estimate_device(pc.frames(name), rots, intrs, terms=0, eng=eng)
        assert not colour.alpha.any() and pc.errors(name, colour.log_gains, colour.alpha)[0] <= CAP


def test_estimate_without_an_overlap(eng, caplog):
    import logging
    rots, intrs = pc.cameras("apart")
    with caplog.at_level(logging.WARNING):
        model = photo.estimate_device(pc.frames("apart"), rots, intrs, eng=eng)
    assert "no camera pair" in caplog.text
    assert not model.log_gains.any() and not model.alpha.any()
    outs = photo.apply_device(pc.frames("apart"), model, eng)
    for out, frame in zip(outs, pc.frames("apart")):
        assert np.array_equal(out.cpu().numpy(), frame)             # gains of 1: the frames themselves


# ------------------------------------------------------------ the correction
def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _model_for(n, seed=3):
    rng = np.random.default_rng(seed)
    return photo.PhotoModel(np.log(rng.uniform(0.7, 1.4, size=(n, 3))), (-0.45, 0.10, 0.03))


def _expected(frames, model):
    return [pm.apply(f, pm.table(lg, model.alpha)) for f, lg in zip(frames, model.log_gains)]


@pytest.mark.parametrize("name", ("rig5", "mixed"))
def test_apply_equals_the_model(eng, name):
    frames = pc.frames(name)
    lg, alpha, _ = pc.estimate(name)
    model = photo.PhotoModel(lg, alpha)
    outs = photo.apply_device(frames, model, eng)
    for k, (out, want) in enumerate(zip(outs, _expected(frames, model))):
        assert out.dtype == torch.uint8 and out.is_contiguous()
        assert np.array_equal(out.cpu().numpy(), want), (name, k)
    again = photo.apply_device(frames, model, eng)
    assert all(torch.equal(a, b) for a, b in zip(outs, again))
    # the corrected frames are closer to each other than the recorded ones
    pairs = list(pc.pairs(name))
    assert pm.overlap_difference([o.cpu().numpy() for o in outs], pairs) < \
        pm.overlap_difference(frames, pairs) / 4


def test_apply_on_noise_small_frames_and_many(eng):
    """Noise (a smooth frame hides a wrong byte), gains above 1 (the clamp to 255), a 1 x 1 and a
    33 x 9 frame (a row's tail, fewer rows than a tile), and 131 frames: more than a launch takes."""
    shapes = [(64, 96), (1, 1), (9, 33), (40, 48), (2, 5)]
    frames = [_noise(h, w, 11 * h + w) for h, w in shapes]
    model = _model_for(len(frames))
    outs = photo.apply_device(frames, model, eng)
    want = _expected(frames, model)
    for k, out in enumerate(outs):
        assert np.array_equal(out.cpu().numpy(), want[k]), shapes[k]
    assert any((w == 255).any() for w in want)
    order = [k % 4 + 1 for k in range(131)]
    many = photo.PhotoModel(model.log_gains[order], model.alpha)
    outs = photo.apply_device([frames[k] for k in order], many, eng)
    for k, out in zip(order, outs):
        assert np.array_equal(out.cpu().numpy(), want[k]), k


def test_apply_pitched_and_in_place(eng):
    """A source that is a rectangle of a larger tensor at an odd base; a pitched destination whose
    surroundings stay; dst == src (through the C ABI: ``apply_device`` allocates its outputs)."""
    h, w = 37, 70
    img = _noise(h, w, 5)
    model = _model_for(1, 9)
    want = _expected([img], model)[0]
    table = torch.from_numpy(photo.tables(model)[0]).to(eng.device)
    big = _noise(h + 9, w + 14, 6)
    big[4:4 + h, 5:5 + w] = img
    dev = torch.from_numpy(big).to(eng.device)
    view = dev[4:4 + h, 5:5 + w]
    assert view.stride(0) > 3 * w and view.data_ptr() % 4 != 0
    outs = photo.apply_device([view], model, eng)
    assert np.array_equal(outs[0].cpu().numpy(), want)
    assert np.array_equal(dev.cpu().numpy(), big)

    def call(src, dst):
        rec = _lib.PhotoApply(src.data_ptr(), dst.data_ptr(), table.data_ptr(), src.stride(0),
                              dst.stride(0), w, h)
        _lib.check(eng.lib.pano_photo_apply_u8(eng.ctx(), C.byref(rec), 1), "pano_photo_apply_u8")
    for x0, extra in ((2, 7), (4, 4)):                  # rows off and on four bytes
        target = torch.full((h + 3, w + extra, 3), 77, dtype=torch.uint8, device=eng.device)
        inner = target[1:1 + h, x0:x0 + w]
        call(view, inner)
        host = target.cpu().numpy()
        assert np.array_equal(host[1:1 + h, x0:x0 + w], want)
        host[1:1 + h, x0:x0 + w] = 77
        assert (host == 77).all()
    # in place: contiguous (dword stores) and pitched at an odd base (bytes)
    same = torch.from_numpy(img.copy()).to(eng.device)
    call(same, same)
    assert np.array_equal(same.cpu().numpy(), want)
    call(view, view)
    host = dev.cpu().numpy()
    assert np.array_equal(host[4:4 + h, 5:5 + w], want)
    host[4:4 + h, 5:5 + w] = img
    assert np.array_equal(host, big)
    # a tensor whose pixels are not contiguous is copied first
    rgba = torch.zeros((h, w, 4), dtype=torch.uint8, device=eng.device)
    rgba[..., :3] = torch.from_numpy(img.copy()).to(eng.device)
    outs = photo.apply_device([rgba[..., :3]], model, eng)
    assert np.array_equal(outs[0].cpu().numpy(), want)


# ------------------------------------------------------------------- error paths
def test_the_abi_refuses_bad_statistics(eng):
    a = torch.full((6, 8, 3), 100, dtype=torch.uint8, device=eng.device)
    b = torch.full((6, 8, 3), 120, dtype=torch.uint8, device=eng.device)
    sums = torch.full((2, 25), 77.0, dtype=torch.float64, device=eng.device)
    inf, nan = float("inf"), float("nan")
    dptr = C.POINTER(C.c_double)
    eye = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)

    def call(frame=None, pair=None, null=(), n_frames=2, n_pairs=2, step=1, lo=16, hi=239,
             lg=(0.0,) * 6, alpha=(0.0,) * 3, tau=inf):
        frames = (_lib.PhotoFrame * 2)(_lib.PhotoFrame(a.data_ptr(), 24, 8, 6),
                                       _lib.PhotoFrame(**dict(dict(img=b.data_ptr(), pitch=24, w=8, h=6),
                                                              **(frame or {}))))
        fields = dict(dict(H=eye, i=0, j=1), **(pair or {}))
        fields["H"] = (C.c_double * 9)(*fields["H"])
        pairs = (_lib.PhotoPair * 2)(_lib.PhotoPair((C.c_double * 9)(*eye), 0, 1), _lib.PhotoPair(**fields))
        lg_arr, alpha_arr = (C.c_double * 6)(*lg), (C.c_double * 3)(*alpha)
        return eng.lib.pano_photo_stats(
            eng.ctx(), None if "frames" in null else frames, n_frames,
            None if "pairs" in null else pairs, n_pairs, step, lo, hi,
            None if "lg" in null else C.cast(lg_arr, dptr),
            None if "alpha" in null else C.cast(alpha_arr, dptr), tau,
            None if "sums" in null else sums.data_ptr())
    for bad in (dict(null=("frames",)), dict(null=("pairs",)), dict(null=("lg",)), dict(null=("alpha",)),
                dict(null=("sums",)), dict(frame=dict(img=None)), dict(n_frames=0), dict(n_pairs=-1),
                dict(frame=dict(w=1)), dict(frame=dict(h=1)), dict(frame=dict(w=32768, pitch=3 * 32768)),
                dict(frame=dict(h=32768)), dict(frame=dict(pitch=23)), dict(step=0), dict(step=-3),
                dict(lo=0), dict(hi=256), dict(lo=200, hi=100), dict(pair=dict(i=-1)),
                dict(pair=dict(j=2)), dict(pair=dict(i=1, j=1)), dict(n_frames=1),
                dict(pair=dict(H=eye[:4] + (nan,) + eye[5:])), dict(pair=dict(H=(inf,) + eye[1:])),
                dict(lg=(0.0, nan, 0.0, 0.0, 0.0, 0.0)), dict(lg=(0.0,) * 5 + (inf,)),
                dict(alpha=(0.0, inf, 0.0)), dict(alpha=(nan, 0.0, 0.0)), dict(tau=nan), dict(tau=0.0),
                dict(tau=-1.0), dict(tau=-inf)):
        assert call(**bad) == _lib.EINVAL, bad
        assert b"pano_photo_stats" in eng.lib.pano_last_error()
    torch.cuda.synchronize()
    assert float(sums.min()) == 77.0 == float(sums.max())           # nothing was launched
    # no pair: nothing to do; the good call: both pairs the same, 48 samples of log(100 / 120)
    assert call(n_pairs=0) == 0
    torch.cuda.synchronize()
    assert float(sums.min()) == 77.0 == float(sums.max())
    assert call(lo=1, hi=255, tau=inf) == 0
    host = sums.cpu().numpy()
    assert np.array_equal(host[0], host[1]) and host[0, 0] == 48.0
    assert np.allclose(host[0, [10, 15, 20]], 48 * np.log(100 / 120), rtol=1e-12)
    assert not host[0, 1:10].any()                                   # the identity: rho_i = rho_j


def test_the_abi_refuses_bad_corrections(eng):
    src = torch.full((6, 8, 3), 9, dtype=torch.uint8, device=eng.device)
    dst = torch.full((6, 8, 3), 77, dtype=torch.uint8, device=eng.device)
    table = torch.ones((3, pm.TABLE), dtype=torch.float32, device=eng.device)
    good = dict(src=src.data_ptr(), dst=dst.data_ptr(), table=table.data_ptr(), src_pitch=24,
                dst_pitch=24, w=8, h=6)

    def call(n=1, null=False, **change):
        recs = (_lib.PhotoApply * 2)(_lib.PhotoApply(**good), _lib.PhotoApply(**dict(good, **change)))
        return eng.lib.pano_photo_apply_u8(eng.ctx(), None if null else recs, n + 1 if n else 0)
    for bad in (dict(n=0), dict(n=-2), dict(null=True), dict(src=None), dict(dst=None), dict(table=None),
                dict(w=0), dict(h=0), dict(w=32768), dict(h=32768), dict(src_pitch=23),
                dict(dst_pitch=23), dict(dst=src.data_ptr() + 24 * 5 + 23), dict(dst=src.data_ptr() + 3),
                dict(src=dst.data_ptr() + 24), dict(dst=src.data_ptr(), dst_pitch=48)):
        assert call(**bad) == _lib.EINVAL, bad
        assert b"pano_photo_apply_u8" in eng.lib.pano_last_error()
    torch.cuda.synchronize()
    assert int(dst.min()) == 77 == int(dst.max())       # nothing was launched, the good record neither
    assert int(src.min()) == 9 == int(src.max())
    # neighbours that do not overlap are taken, and so is dst == src
    both = torch.full((12, 8, 3), 5, dtype=torch.uint8, device=eng.device)
    assert call(src=both.data_ptr(), dst=both.data_ptr() + 6 * 24) == 0
    assert call(src=both.data_ptr(), dst=both.data_ptr()) == 0
    torch.cuda.synchronize()
    assert int(both.min()) == 5 == int(both.max()) and int(dst.min()) == 9 == int(dst.max())


# -------------------------------------------------------------------- end to end
def test_cli_photometric(eng, tmp_path, monkeypatch):
    import bundle_adj
    import stitcher as top
    from PIL import Image
    name = "rig5"
    rots, intrs = pc.cameras(name)
    rig = tmp_path / "RIG"
    rig.mkdir()
    for i, im in enumerate(pc.frames(name)):
        Image.fromarray(np.ascontiguousarray(im[..., ::-1])).save(rig / f"frame{i}.png")
    files = [f for f in os.listdir(rig) if f.endswith(".png")]
    order = [int(f[5:-4]) for f in files]               # the ingest reads in os.listdir order

    def cameras():
        return [bundle_adj.Image(None, rots[i], intrs[i]) for i in order]
    with open(tmp_path / "ba_RIG_s1.0.pkl", "wb") as fid:
        pickle.dump(cameras(), fid, protocol=pickle.HIGHEST_PROTOCOL)
    monkeypatch.chdir(tmp_path)
    raw = top.ingest(str(rig), 1)
    for i, frame in zip(order, raw):
        assert np.array_equal(frame.cpu().numpy(), pc.frames(name)[i])

    def stitched(frames, terms):
        regions = cameras()
        for reg, frame in zip(regions, frames):
            reg.img = frame
        if terms is not None:
            model = photo.correct_regions(regions, terms)
            assert all(isinstance(reg.img, torch.Tensor) and reg.img.is_cuda for reg in regions)
            assert all(not np.array_equal(reg.img.cpu().numpy(), pc.frames(name)[i])
                       for reg, i in zip(regions, order))
            if terms == 2:
                assert np.abs(model.log_gains - pc.truth(name)[0][order]).max() <= CAP
        return top.stitch(regions, blender=top.linear_blend)
    got = {}
    for mode, terms in photo.MODES.items():
        got[mode] = top.main([str(rig), "--photometric", mode, "-b", "linear", "-s", "1"])
        assert np.array_equal(got[mode], stitched(raw, terms)), mode
    assert not np.array_equal(got["color"], got["vignette"])
    # host arrays in the regions (a cache that carries pixels) give the same mosaic
    assert np.array_equal(got["vignette"], stitched([f.cpu().numpy() for f in raw], 2))
    # without the flag: what it returned before - the stitch of the raw frames
    plain = top.main([str(rig), "-b", "linear", "-s", "1"])
    assert np.array_equal(plain, stitched(raw, None))
    assert plain.shape == got["vignette"].shape and not np.array_equal(plain, got["vignette"])
    assert sorted(os.listdir(tmp_path)) == ["RIG", "ba_RIG_s1.0.pkl"]     # no other cache appeared
