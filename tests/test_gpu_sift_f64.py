"""GPU: the SIFT front end stage by stage through the C ABI against the float64 restatement
(tests/sift_f64.py).  Every stage reads float32 inputs that the truth reads too - the kernel's own
previous layer, its own DoG planes, keypoint records built on the host - and is judged as
tests/test_gpu_float64_truth.py judges the blend: the kernel within the bound E, the float32
oracle within E on the same items, the kernel's worst at most 4 x the oracle's, and every decided
discrete outcome the same.  Lists filled by atomics are compared as sets."""
import ctypes as C
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_f64 as sf  # noqa: E402

pytestmark = pytest.mark.gpu


def _kp_dtype():
    from pano360_amd import features
    return features.KP_DTYPE


def _pyramid(eng, bgr, layers):
    """``features.sift_pyramid_device`` of ``bgr``: (gauss, dog) on the host, the step taps, and
    the device stacks."""
    import torch
    from pano360_amd import features
    frame = torch.from_numpy(np.ascontiguousarray(bgr)).to(eng.device)
    g_dev, d_dev = features.sift_pyramid_device(frame, layers=layers, eng=eng)
    sig_diff = float(np.sqrt(max(np.float32(1.6) ** 2 - np.float32(0.5) ** 2 * 4, np.float32(0.01))))
    kernels = [features._step_taps(s) for s in [sig_diff] + features.sift_sigmas(1.6, layers)[1:]]
    return [g.cpu().numpy() for g in g_dev], [d.cpu().numpy() for d in d_dev], kernels, (g_dev, d_dev)


def _tables(eng, gauss_dev):
    """The plane and dimension tables as SiftPipeline._slot builds them: 256 entries, zero planes
    beyond the pyramid."""
    import torch
    dims = np.zeros((256, 2), np.int32)
    dims[:len(gauss_dev)] = [tuple(g.shape[1:]) for g in gauss_dev]
    gptr = np.zeros(256, np.int64)
    gptr[:len(gauss_dev)] = [g.data_ptr() for g in gauss_dev]
    return (torch.from_numpy(dims.reshape(-1)).to(eng.device),
            torch.from_numpy(gptr).to(eng.device))


# ------------------------------------------------------------------------ a. scale space
# octave 0 of 140 x 264: interior tiles with w % 4 == 0 (the 16-byte staging); octave 1 132
# columns (w % 4 == 0 again, narrower), 66 (w % 4 == 2: float2 stores), 33 (odd: scalar stores),
# and octaves under 32 rows / 64 columns
SHAPES = [(70, 132), (45, 61)]


@pytest.mark.parametrize("layers", [3, 4, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_scale_space_one_step_at_a_time(eng, layers, shape):
    """G_i against step_f64 of the kernel's own G_{i-1}; layer 0 against step_f64 of up2(grey) in
    float64 (the grey conversion and the upsampling judged with it); the oracle's float32 step of
    the same input within the same bound; DoG_{i-1} = G_i - G_{i-1} of the stored layers bit for
    bit; each octave's base the exact decimation of layer ``layers``."""
    import cv2_shim
    import sift_pyramid as sp
    from pano360_amd import synth
    h, w = shape
    bgr = synth.make_frame(11, w, h, "B")
    gauss, dog, taps, _ = _pyramid(eng, bgr, layers)
    base64 = sf.up2_f64(sp.gray_u8(bgr))
    worst_k = worst_o = 0.0
    for o in range(len(gauss)):
        if o:
            assert np.array_equal(gauss[o][0], sp.decimate2(gauss[o - 1][layers])), o
        for i in range(0 if o == 0 else 1, layers + 3):
            src = base64 if i == 0 else gauss[o][i - 1]
            truth = sf.step_f64(src, taps[i])
            E = sf.step_bound(len(taps[i])) + (4 if i == 0 else 0)
            if i == 0:
                src = sp.resize_up2(sp.gray_u8(bgr))             # the oracle's own float32 base
            ek = sf.step_error(gauss[o][i], truth).max()
            eo = sf.step_error(cv2_shim.sep_filter_symm(src, taps[i]), truth).max()
            assert ek <= E and eo <= E, (o, i, ek, eo, E)
            worst_k, worst_o = max(worst_k, ek / E), max(worst_o, eo / E)
            if i:
                assert np.array_equal(dog[o][i - 1], gauss[o][i] - gauss[o][i - 1]), (o, i)
    assert worst_k <= 4 * worst_o, (worst_k, worst_o)
    print(f"scale space {shape} layers {layers}: kernel worst e/E {worst_k:.3f}, oracle {worst_o:.3f}, "
          f"{len(gauss)} octaves, undecided 0")


@pytest.mark.parametrize("ntaps", [1, 3, 9, 31, 33])
@pytest.mark.parametrize("shape", [(37, 70), (64, 128), (3, 5)])
def test_scale_step_apertures(eng, ntaps, shape):
    """pano_scale_step called directly at apertures outside the five templates (the looped form),
    its DoG output and REFLECT_101 on planes narrower than the radius."""
    import cv2_shim
    import torch
    from pano360_amd import _lib, engine
    from pano360_amd.engine import _ptr
    rng = np.random.default_rng(ntaps * 7 + shape[1])
    src = (rng.random(shape) * 255).astype(np.float32)
    taps = engine.gaussian_taps(ntaps, max((ntaps - 1) / 8.0, 0.3)).astype(np.float32)
    dsrc = torch.from_numpy(src).to(eng.device)
    out = torch.empty_like(dsrc)
    dog = torch.empty_like(dsrc)
    _lib.check(eng.lib.pano_scale_step(eng.ctx(), _ptr(dsrc), shape[0], shape[1], taps.ctypes.data,
                                       ntaps, _ptr(out), _ptr(dog)), "pano_scale_step")
    got = out.cpu().numpy()
    truth = sf.step_f64(src, taps)
    E = sf.step_bound(ntaps)
    ek = sf.step_error(got, truth).max()
    eo = sf.step_error(cv2_shim.sep_filter_symm(src, taps), truth).max()
    assert ek <= E and eo <= E and ek <= 4 * max(eo, 1.0), (ek, eo, E)
    assert np.array_equal(dog.cpu().numpy(), got - src)


def test_scale_step_argument_checks(eng):
    """Aperture 35 is refused with the library's error, and so is a 2-layer scale space (its last
    step needs 37 taps)."""
    import torch
    from pano360_amd import _lib, features
    from pano360_amd.engine import _ptr
    src = torch.zeros((40, 40), dtype=torch.float32, device=eng.device)
    out = torch.empty_like(src)
    taps = np.full(35, 1.0 / 35, np.float32)
    with pytest.raises(_lib.PanoError, match="aperture 35"):
        _lib.check(eng.lib.pano_scale_step(eng.ctx(), _ptr(src), 40, 40, taps.ctypes.data, 35,
                                           _ptr(out), None), "pano_scale_step")
    frame = torch.zeros((40, 40, 3), dtype=torch.uint8, device=eng.device)
    with pytest.raises(_lib.PanoError, match="aperture 37"):
        features.sift_pyramid_device(frame, layers=2, eng=eng)


def test_pipeline_pyramid_of_four_layers_eager_captured_and_replayed(eng):
    """SiftPipeline(layers=4).pyramid(): launch by launch, captured and replayed, the same scale
    space as the entry points."""
    import torch
    from pano360_amd import _lib, engine, features, synth
    h, w = 60, 84
    frame = torch.from_numpy(synth.make_frame(5, w, h, "B")).to(eng.device)
    g_ref, d_ref = features.sift_pyramid_device(frame, layers=4, eng=eng)
    use = engine.Engine(eng.device)
    use.set_option(_lib.OPT_SIFT_GRAPH, 1)
    pipe = features.SiftPipeline(use, h, w, depth=1, layers=4)
    for _ in range(3):
        gauss, dog = pipe.pyramid(frame)
        torch.cuda.synchronize(eng.device)
        assert all(torch.equal(a, b) for a, b in zip(gauss, g_ref))
        assert all(torch.equal(a, b) for a, b in zip(dog, d_ref))


# ------------------------------------------------------------------------ b. extrema
def _extrema_dev(eng, dog, octave, n_layers, max_cands=1 << 16):
    """pano_sift_extrema on a host DoG stack: (records, the device count)."""
    import torch
    from pano360_amd import _lib
    from pano360_amd.engine import _ptr
    d = torch.from_numpy(np.ascontiguousarray(dog, np.float32)).to(eng.device)
    cands = torch.zeros(max_cands * 32, dtype=torch.uint8, device=eng.device)
    count = torch.zeros(1, dtype=torch.int32, device=eng.device)
    _, rows, cols = dog.shape
    _lib.check(eng.lib.pano_sift_extrema(eng.ctx(), _ptr(d), rows, cols, octave, n_layers, 0.04,
                                         10.0, 1.6, _ptr(cands), _ptr(count), max_cands),
               "pano_sift_extrema")
    n = int(count.item())
    return cands[:min(n, max_cands) * 32].cpu().numpy().view(_kp_dtype()), n


def _judge_extrema(got, dog, octave, n_layers, oracle=True):
    """Decided float64 survivors one to one with the kernel's (keys layer, r, c), values within
    bound; returns (kernel worst e, oracle worst e, undecided, total)."""
    import sift_oracle as so
    cands = sf.extrema(dog, n_layers)
    res = sf.refine_f64(dog, octave, cands, n_layers)
    und = ~res["decided"]
    key = lambda l, r, c: (int(l), int(r), int(c))  # noqa: E731
    unsure = Counter(key(res["layer"][k], res["r"][k], res["c"][k]) for k in np.nonzero(und)[0])
    sure = {}
    for k in np.nonzero(res["kept"] & res["decided"])[0]:
        sure.setdefault(key(res["layer"][k], res["r"][k], res["c"][k]), []).append(k)
    gk = {}
    for rec in got:
        gk.setdefault(key((rec["octave"] >> 8) & 255, rec["r"], rec["c"]), []).append(rec)
    # a kernel record the decided survivors do not explain must come from an undecided candidate:
    # within one pixel and layer of where that candidate's Newton steps went
    reach = set()
    for k in np.nonzero(und)[0]:
        for p in {tuple(int(v) for v in q) for q in res["path"][k]}:
            reach.update((p[0] + a, p[1] + b, p[2] + c)
                         for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1))
    extra = [k for k in gk if k not in sure]
    assert all(k in reach for k in extra), [k for k in extra if k not in reach][:5]
    worst_k = worst_o = 0.0
    worst_at = None
    for kk, idx in sure.items():
        recs = gk.get(kk, [])
        if kk in unsure:
            continue
        assert len(recs) == len(idx), (kk, len(recs), len(idx))
        for rec in recs:
            # several candidates may converge on one pixel: the closest truth
            errs = []
            for k in idx:
                e = max(abs(float(rec["x"]) - res["x"][k]) / res["dx"][k],
                        abs(float(rec["y"]) - res["y"][k]) / res["dy"][k],
                        abs(float(rec["size"]) - res["size"][k]) / res["dsize"][k],
                        abs(float(rec["response"]) - res["response"][k]) / res["dresp"][k])
                mask = -1 if res["oct_decided"][k] else 0xffff
                if int(rec["octave"]) & mask == int(res["octave"][k]) & mask:
                    errs.append(e)
            assert errs and min(errs) <= 1.0, (kk, errs)
            if min(errs) >= worst_k:
                worst_k, worst_at = min(errs), idx

    if oracle:
        # the oracle on the items of the kernel's worst, 400 decided survivors spread over the
        # octave and 100 decided rejections
        planes = list(np.asarray(dog, np.float32))
        kept = np.nonzero(res["kept"] & res["decided"])[0]
        gone = np.nonzero(~res["kept"] & res["decided"])[0]
        pick = set(kept[::max(1, len(kept) // 400)]) | set(gone[:100]) | set(worst_at or [])
        for k in sorted(pick):
            kp = so.adjust_local_extrema(planes, octave, *map(int, cands[k]), n_layers)
            assert (kp is not None) == res["kept"][k]
            if kp is not None:
                worst_o = max(worst_o, abs(float(kp["x"]) - res["x"][k]) / res["dx"][k],
                              abs(float(kp["y"]) - res["y"][k]) / res["dy"][k],
                              abs(float(kp["size"]) - res["size"][k]) / res["dsize"][k],
                              abs(float(kp["response"]) - res["response"][k]) / res["dresp"][k])
        assert worst_o <= 1.0
    return worst_k, worst_o, int(und.sum()), len(cands)


@pytest.mark.parametrize("layers,shape", [(3, (40, 67)), (3, (36, 133)), (3, (30, 135)),
                                          (4, (70, 132)), (5, (45, 61))])
def test_extrema_against_f64(eng, layers, shape):
    """pano_sift_extrema on the kernel's own DoG stacks: the streaming search at 3 layers (octave
    interiors of 62 k (octave 0 of w = 67), 62 k - 1 and 62 k + 1 columns (octave 1 of w = 133, 135), short last row segments, octaves of 10 rows
    or fewer that give none) and the general kernel at 4 and 5 layers."""
    from pano360_amd import synth
    h, w = shape
    _, dog, _, _ = _pyramid(eng, synth.make_frame(21, w, h, "B"), layers)
    wk = wo = 0.0
    und = tot = 0
    for o, d in enumerate(dog):
        got, n = _extrema_dev(eng, d, o, layers)
        if min(d.shape[1:]) <= 10:
            assert n == 0
            continue
        k, oo, u, t = _judge_extrema(got, d, o, layers)
        wk, wo, und, tot = max(wk, k), max(wo, oo), und + u, tot + t
    assert tot > 30 and und <= 0.05 * tot, (und, tot)
    assert wk <= 4 * max(wo, 0.05), (wk, wo)
    print(f"extrema {shape} layers {layers}: kernel worst e/E {wk:.3f}, oracle {wo:.3f}, "
          f"undecided {und}/{tot}")


def test_extrema_wide_octave_and_overflow(eng):
    """A 3-layer DoG stack 16400 columns wide takes the general kernel (every frame 8192 px or wider
    does at octave 0); a dense noise stack flushes the scan's LDS list many times; a capacity below
    the candidate count reports the overflow and stores genuine candidates only."""
    rng = np.random.default_rng(4)
    wide = (rng.standard_normal((5, 24, 16400)) * 4).astype(np.float32)
    got, n = _extrema_dev(eng, wide, 0, 3, max_cands=1 << 18)
    wk, wo, und, tot = _judge_extrema(got, wide, 0, 3)
    assert n == len(got) and tot > 1000
    dense = (rng.standard_normal((5, 300, 257)) * 4).astype(np.float32)
    got, n = _extrema_dev(eng, dense, 1, 3, max_cands=1 << 18)
    wk2, wo2, und2, tot2 = _judge_extrema(got, dense, 1, 3)
    assert tot2 > 2000
    # overflow: the count goes past the capacity, the stored entries are all genuine
    part, n_over = _extrema_dev(eng, dense, 1, 3, max_cands=len(got) // 2)
    assert n_over > len(got) // 2 and len(part) == len(got) // 2
    full = Counter((int(r["r"]), int(r["c"]), int(r["octave"])) for r in got)
    for rec in part:
        assert full[(int(rec["r"]), int(rec["c"]), int(rec["octave"]))] > 0
    print(f"extrema wide: kernel worst e/E {wk:.3f}, oracle {wo:.3f}, undecided {und}/{tot}; dense: kernel "
          f"{wk2:.3f}, oracle {wo2:.3f}, undecided {und2}/{tot2}")


def test_extrema_pivot_between_one_and_ten_flt_epsilon(eng):
    """A forged DoG whose Hessian's third pivot (the scale curvature nearly cancelled by the
    column-scale cross term) lies between FLT_EPSILON and 10 FLT_EPSILON: singular by the threshold
    of OpenCV's float LU, so the Newton offset is zero and the maximum is kept where it is - the
    kernel, the oracle and the float64 restatement agree.  (A solve that went on below 10
    FLT_EPSILON would step far along scale and drop it.)"""
    import sift_oracle as so
    d = np.zeros((5, 21, 21), np.float32)
    d[2, 10, 10] = 8.0
    d[2, 10, 9] = d[2, 10, 11] = d[2, 9, 10] = d[2, 11, 10] = 4.0
    d[1, 10, 10], d[3, 10, 10] = np.float32(7.901822566986084), np.float32(7.96)
    d[3, 10, 11] = d[1, 10, 9] = np.float32(2.10375)
    piv = np.abs(sf.lu_pivots(sf._derivs(d.astype(np.float64), np.array([2]), np.array([10]),
                                         np.array([10]))[3]))
    assert sf.FLT_EPSILON < piv.min() < sf.PIVOT_EPS
    res = sf.refine_f64(d, 0, np.array([[2, 10, 10]]), 3)
    assert res["decided"][0] and res["kept"][0] and res["x"][0] == res["y"][0] == 10.0
    kp = so.adjust_local_extrema(list(d), 0, 2, 10, 10)
    got, n = _extrema_dev(eng, d, 0, 3)
    assert n == 1 and kp is not None
    assert float(got["x"][0]) == float(kp["x"]) == 10.0 and float(got["y"][0]) == 10.0
    assert int(got["octave"][0]) == int(res["octave"][0]) == kp["octave"]


# ------------------------------------------------------------------------ c. orientation
def _orient_dev(eng, tables, recs, max_kpts=4096):
    import torch
    from pano360_amd import _lib
    from pano360_amd.engine import _ptr
    dims, gptr = tables
    cands = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(eng.device)
    n_c = torch.tensor([len(recs)], dtype=torch.int32, device=eng.device)
    kpts = torch.zeros(max_kpts * 32, dtype=torch.uint8, device=eng.device)
    count = torch.zeros(1, dtype=torch.int32, device=eng.device)
    _lib.check(eng.lib.pano_sift_orient(eng.ctx(), _ptr(gptr), _ptr(dims), 3, _ptr(cands), _ptr(n_c),
                                        len(recs), _ptr(kpts), _ptr(count), max_kpts), "pano_sift_orient")
    n = int(count.item())
    assert n <= max_kpts
    return kpts[:n * 32].cpu().numpy().view(_kp_dtype())


def _judge_orientation(eng, gauss, g_dev, recs):
    """pano_sift_orient on host-built ``recs`` (the response numbers the record) against
    orientation_f64, the oracle's angles of the same records judged alike.  Returns (kernel worst
    e/E, oracle worst e/E, undecided peaks, peaks, records with several decided peaks)."""
    import sift_oracle as so
    recs = np.array(recs, _kp_dtype())
    recs["response"] = np.arange(len(recs), dtype=np.float32) + 1
    out = _orient_dev(eng, _tables(eng, g_dev), recs)
    by = {}
    for rec in out:
        by.setdefault(int(rec["response"]) - 1, []).append(float(rec["angle"]))
    worst = {"kernel": 0.0, "oracle": 0.0}
    und = tot = multi = 0
    for i, rec in enumerate(recs):
        o, layer = int(rec["octave"]) & 255, (int(rec["octave"]) >> 8) & 255
        img, r, c, size = gauss[o][layer], int(rec["r"]), int(rec["c"]), rec["size"]
        peaks = sf.orientation_f64(img, r, c, float(size), o)
        multi += sum(dec for _, _, dec in peaks) > 1
        for who, angles in (("kernel", by.get(i, [])),
                            ("oracle", [float(a) for a in so.orientation_angles(img, r, c, size, o)])):
            for a, da, dec in peaks:
                tot += who == "kernel"
                if not dec:
                    und += who == "kernel"
                    continue
                dd = [abs((g - a + 180.0) % 360.0 - 180.0) for g in angles]
                assert dd and min(dd) <= da, (who, i, a, da, angles)
                worst[who] = max(worst[who], min(dd) / da)
            for g in angles:
                assert any(abs((g - a + 180.0) % 360.0 - 180.0) <= da for a, da, _ in peaks), (who, i, g)
    assert worst["kernel"] <= 4 * max(worst["oracle"], 0.01), worst
    return worst["kernel"], worst["oracle"], und, tot, multi


def test_orientation_against_f64(eng):
    """pano_sift_orient on records built on the host: the kernel's own candidates, windows cut by
    every border, the largest radius a layer allows."""
    from pano360_amd import synth
    h, w = 64, 96
    gauss, dog, _, (g_dev, _) = _pyramid(eng, synth.make_frame(31, w, h, "B"), 3)
    recs = []
    for o in range(3):
        got, _ = _extrema_dev(eng, dog[o], o, 3)
        recs += list(got[:60])
    rows, cols = gauss[1].shape[1:]
    for r, c, size in ((1, 1, 8.0), (0, cols - 1, 6.0), (rows - 2, 3, 12.0), (rows - 1, cols // 2, 4.0),
                       (rows // 2, cols // 2, 2.0 * rows * 2 / 4.5)):
        rec = np.zeros(1, _kp_dtype())[0]
        rec["r"], rec["c"], rec["size"], rec["octave"] = r, c, size, 1 | (2 << 8)
        recs.append(rec)
    wk, wo, und, tot, _ = _judge_orientation(eng, gauss, g_dev, recs)
    assert tot > 100 and und <= 0.05 * tot, (und, tot)
    print(f"orientation: kernel worst e/E {wk:.3f}, oracle {wo:.3f}, undecided {und}/{tot}")


def _forged(eng, plane, layers=3):
    """A one-octave pyramid whose every Gaussian layer is ``plane`` (host and device)."""
    import torch
    stack = np.repeat(np.asarray(plane, np.float32)[None], layers + 3, axis=0)
    return [stack], [torch.from_numpy(stack).to(eng.device)]


def test_orientation_of_forged_planes_with_several_peaks(eng):
    """Histograms with two and three peaks of equal height (planes that are the maximum of two or
    three ramps meeting at the keypoint) and a +-255 checkerboard of period 4, every decided peak
    found with its angle within bound."""
    yy, xx = np.mgrid[:64, :64].astype(np.float64) - 32.0
    planes = [100 + 2 * np.maximum(xx, yy),
              100 + 2 * np.maximum.reduce([xx, -0.5 * xx + 0.8660254 * yy, -0.5 * xx - 0.8660254 * yy]),
              255.0 * (((np.arange(64)[:, None] // 2) + (np.arange(64)[None] // 2)) % 2)]
    multi = 0
    for plane in planes:
        gauss, g_dev = _forged(eng, plane)
        recs = []
        for r, c, size in ((32, 32, 6.0), (32, 32, 10.0), (31, 33, 3.0), (2, 60, 8.0)):
            rec = np.zeros(1, _kp_dtype())[0]
            rec["r"], rec["c"], rec["size"], rec["octave"] = r, c, size, 0 | (1 << 8)
            recs.append(rec)
        wk, wo, und, tot, m = _judge_orientation(eng, gauss, g_dev, recs)
        multi += m
        print(f"orientation, forged plane: kernel worst e/E {wk:.3f}, oracle {wo:.3f}, undecided "
              f"{und}/{tot}, records with several decided peaks {m}")
    assert multi >= 4, multi


# ------------------------------------------------------------------------ d. descriptors
def _describe_dev(eng, tables, recs):
    import torch
    from pano360_amd import _lib
    from pano360_amd.engine import _ptr
    dims, gptr = tables
    kp = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(eng.device)
    desc = torch.zeros((len(recs), 128), dtype=torch.float32, device=eng.device)
    _lib.check(eng.lib.pano_sift_describe(eng.ctx(), _ptr(gptr), _ptr(dims), -1, _ptr(kp), len(recs),
                                          None, _ptr(desc)), "pano_sift_describe")
    return desc.cpu().numpy()


def test_descriptors_against_f64(eng):
    """pano_sift_describe on hand-placed keypoints - octave -1, 0 and coarse octaves smaller than
    the window; positions on and next to every edge; angles 0, 1e-4, 90, 180, 359.999 and 45
    (most samples of a diagonal ramp on |dx| = |dy|); sizes across several fixed-point units - and
    on the kernel's own detections: every entry within 0.5 + delta of the real-valued truth."""
    import torch
    from pano360_amd import features, synth
    h, w = 48, 80
    bgr = synth.make_frame(41, w, h, "B")
    yy, xx = np.mgrid[:h, :w]
    bgr[:h // 4] = np.clip((xx + yy)[:h // 4] * 3, 0, 255).astype(np.uint8)[..., None]   # diagonal ramp
    gauss, _, _, (g_dev, d_dev) = _pyramid(eng, bgr, 3)
    tables = _tables(eng, g_dev)
    recs = []
    for o in range(len(gauss)):                            # octave byte o - 1 (first octave -1)
        rows, cols = gauss[o].shape[1:]
        s = 2.0 ** (o - 1)
        for py in sorted({0, 1, rows // 2, rows - 2, rows - 1}):
            for px in sorted({0, 1, cols // 3, cols - 2, cols - 1}):
                for angle, size in ((0.0, 3.2), (1e-4, 5.0), (90.0, 9.0), (180.0, 17.0),
                                    (359.999, 40.0), (45.0, 2.0)):
                    rec = np.zeros(1, _kp_dtype())[0]
                    rec["x"], rec["y"], rec["size"], rec["angle"] = px * s, py * s, size * s, angle
                    rec["octave"] = ((o - 1) & 255) | ((1 + (px + py) % 3) << 8)
                    recs.append(rec)
    frame = torch.from_numpy(bgr).to(eng.device)
    kps, _ = features.sift_detect_device(frame, pyramid=(g_dev, d_dev), eng=eng)
    recs = np.concatenate([np.array(recs, _kp_dtype()), kps[:300]])
    got = _describe_dev(eng, tables, recs)
    worst = 0.0
    near = 0
    for rec, row in zip(recs, got):
        octave, layer = sf.unpack_octave(int(rec["octave"]))
        v, delta = sf.descriptor_f64(gauss[octave + 1][layer], rec["x"], rec["y"], rec["size"],
                                     rec["angle"], int(rec["octave"]))
        err = np.abs(row - np.clip(v, 0, 255))
        assert (err <= 0.5 + delta).all(), (rec, float((err - 0.5 - delta).max()))
        worst = max(worst, float(err.max()))
        near += int(sf._near_half(v, delta).sum())
    assert near <= 0.05 * got.size
    print(f"descriptors: {len(recs)} keypoints, kernel worst |got - v| {worst:.3f} (E 0.5 + delta), "
          f"undecided entries {near}/{got.size}")


def test_descriptors_of_maximal_gradients_at_the_fixed_point_extremes(eng):
    """Forged Gaussian planes whose central differences are all +-255: stripes of period 4 (|dx| =
    255, two orientations: half the samples in each bin pair) and a checkerboard of 2 x 2 blocks
    (|dx| = |dy| = 255, |grad| = 361, the largest there is).  Keypoints at the smallest scales
    (kbits 17: a bin's 36 samples of 361 come to 80 % of a 32-bit half) up to kbits 0, each
    descriptor entry within 0.5 + delta of the truth."""
    n = np.arange(64)
    stripes = np.tile(255.0 * ((n // 2) % 2), (64, 1))
    checker = 255.0 * (((n[:, None] // 2) + (n[None] // 2)) % 2)
    worst = 0.0
    kbits_seen = set()
    for plane in (stripes, checker):
        gauss, g_dev = _forged(eng, plane)
        recs = []
        for scl in (0.5, 1.0, 1.7, 6.0, 40.0, 500.0):        # kbits 17, 17, 16, 12, 5, 0
            for px, py, angle in ((32, 32, 0.0), (31, 33, 30.0), (2, 61, 135.0)):
                rec = np.zeros(1, _kp_dtype())[0]
                # octave byte 255 (-1): full-resolution coordinates are half the plane's
                rec["x"], rec["y"], rec["size"], rec["angle"] = px / 2, py / 2, scl, angle
                rec["octave"] = 255 | (1 << 8)
                recs.append(rec)
                kb = 31 - int(np.ceil(np.log2(np.float32(36.0) * np.float32(max(scl * scl, 1.0))
                                              * np.float32(361.0))))
                kbits_seen.add(min(max(kb, 0), 24))
        recs = np.array(recs, _kp_dtype())
        got = _describe_dev(eng, _tables(eng, g_dev), recs)
        for rec, row in zip(recs, got):
            v, delta = sf.descriptor_f64(gauss[0][1], rec["x"], rec["y"], rec["size"], rec["angle"],
                                         int(rec["octave"]))
            err = np.abs(row - np.clip(v, 0, 255))
            assert (err <= 0.5 + delta).all(), (rec, float((err - 0.5 - delta).max()))
            assert row.max() > 0
            worst = max(worst, float(err.max()))
    assert {0, 17} <= kbits_seen
    print(f"descriptors of +-255 planes: kbits {sorted(kbits_seen)}, kernel worst |got - v| {worst:.3f}")


# ------------------------------------------------------------------------ e. end to end
@pytest.mark.parametrize("shape,seed", [((64, 96), 51), ((72, 80), 52)])
def test_end_to_end_against_f64(eng, shape, seed):
    """features.sift_detect_device on the kernel's own pyramid: every decided float64 keypoint
    (decided refinement, decided orientation peak) present after the first-octave adjustment, the
    list in OpenCV's order (removeDuplicatedSorted's keys), and every descriptor within 0.5 +
    delta of its truth."""
    from pano360_amd import features, synth
    h, w = shape
    bgr = synth.make_frame(seed, w, h, "B")
    gauss, dog, _, pyr = _pyramid(eng, bgr, 3)
    import torch
    frame = torch.from_numpy(bgr).to(eng.device)
    kps, desc = features.sift_detect_device(frame, pyramid=pyr, eng=eng)
    desc = desc.cpu().numpy()
    # OpenCV's order: the list sorted (before the adjustment) is the list itself
    raw = kps.copy()
    raw["octave"] = (raw["octave"] & ~255) | ((raw["octave"] + 1) & 255)
    for key in ("x", "y", "size"):
        raw[key] = raw[key] * np.float32(2.0)
    resorted = features.sift_sort_unique(raw.copy())
    assert len(resorted) == len(raw)
    for key in ("x", "y", "size", "angle", "response", "octave"):
        assert np.array_equal(resorted[key], raw[key]), key
    want = und = 0
    for o in range(len(dog)):
        stack = dog[o]
        res = sf.refine_f64(stack, o, sf.extrema(stack, 3), 3)
        for k in np.nonzero(res["kept"] & res["decided"])[0]:
            for angle, da, dec in sf.orientation_f64(gauss[o][int(res["layer"][k])], int(res["r"][k]),
                                                     int(res["c"][k]), res["size"][k], o):
                if not dec:
                    und += 1
                    continue
                want += 1
                near = ((np.abs(kps["x"] - 0.5 * res["x"][k]) <= 0.5 * res["dx"][k]) &
                        (np.abs(kps["y"] - 0.5 * res["y"][k]) <= 0.5 * res["dy"][k]) &
                        (np.abs(kps["size"] - 0.5 * res["size"][k]) <= 0.5 * res["dsize"][k]) &
                        (np.abs((kps["angle"] - angle + 180.0) % 360.0 - 180.0) <= da) &
                        ((kps["octave"] & 0xff00) == (int(res["octave"][k]) & 0xff00)) &
                        ((kps["octave"] & 255) == ((o - 1) & 255)))
                assert near.any(), (o, res["r"][k], res["c"][k], angle)
    assert want > 50 and und <= 0.03 * want, (want, und)
    worst = 0.0
    for rec, row in zip(kps, desc):
        octave, layer = sf.unpack_octave(int(rec["octave"]))
        v, delta = sf.descriptor_f64(gauss[octave + 1][layer], rec["x"], rec["y"], rec["size"],
                                     rec["angle"], int(rec["octave"]))
        err = np.abs(row - np.clip(v, 0, 255))
        assert (err <= 0.5 + delta).all(), (rec, float((err - 0.5 - delta).max()))
        worst = max(worst, float(err.max()))
    print(f"end to end {shape}: {want} decided keypoints found among {len(kps)}, {und} undecided "
          f"peaks, descriptors worst |got - v| {worst:.3f}")


def test_extrema_of_a_4k_frame(eng):
    """Octaves 0 and 1 of a 3840 x 2160 frame: octave 0 (7680 columns) is scanned in 96-row
    segments, octave 1 in 24-row ones.  The float64 refinement of every candidate is batched."""
    from pano360_amd import synth
    h, w = 2160, 3840
    _, d_dev = _pyramid_dog_only(eng, synth.make_frame(61, w, h, "B"))
    for o, seg in ((0, 96), (1, 24)):
        d = d_dev[o].cpu().numpy()
        rows, cols = d.shape[1:]
        n_seg = 96
        while n_seg > 12 and -(-(cols - 10) // 62) * -(-(rows - 10) // n_seg) < 4096:
            n_seg //= 2
        assert n_seg == seg
        got, n = _extrema_dev(eng, d, o, 3, max_cands=1 << 20)
        wk, wo, und, tot = _judge_extrema(got, d, o, 3)
        assert tot > 5000 and und <= 0.02 * tot, (und, tot)
        assert wk <= 4 * max(wo, 0.05), (wk, wo)
        print(f"extrema 4K octave {o} ({seg}-row segments): kernel worst e/E {wk:.3f}, oracle "
              f"{wo:.3f}, undecided {und}/{tot}")
        del d


def _pyramid_dog_only(eng, bgr):
    import torch
    from pano360_amd import features
    frame = torch.from_numpy(np.ascontiguousarray(bgr)).to(eng.device)
    return features.sift_pyramid_device(frame, n_octaves=2, eng=eng)


# ------------------------------------------------------------------------ the Python path
def test_detect_async_searches_the_pyramids_layers(eng):
    """sift_detect_async(pyramid=...) of a 4-layer pyramid searches DoG layers 1 - 4 with the
    4-layer sizes (a keypoint in layer 4 exists, each size follows sigma 2^((layer + xi) / 4));
    a pyramid whose octaves disagree on the depth is refused."""
    import torch
    from pano360_amd import features, synth
    frame = torch.from_numpy(synth.make_frame(9, 96, 64, "B")).to(eng.device)
    gauss, dog = features.sift_pyramid_device(frame, layers=4, eng=eng)
    kps, desc = features.sift_detect_device(frame, pyramid=(gauss, dog), eng=eng)
    layer = (kps["octave"] >> 8) & 255
    assert len(kps) > 20 and layer.max() == 4 and layer.min() >= 1
    octave = kps["octave"] & 255
    octave = np.where(octave >= 128, octave - 256, octave)
    xi = ((kps["octave"] >> 16) & 255) / 255.0 - 0.5
    want = 1.6 * 2.0 ** ((layer + xi) / 4.0) * 2.0 ** (octave + 1)     # (halved: first octave -1)
    assert np.allclose(kps["size"], want, rtol=3e-3)
    with pytest.raises(ValueError):
        features.sift_detect_async(frame, pyramid=(gauss, [dog[0]] + [d[:-1] for d in dog[1:]]),
                                   eng=eng)
