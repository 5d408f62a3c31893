"""CPU: the float64 restatement of the SIFT front end (tests/sift_f64.py) checked as a yardstick -
its scale step against a direct tap loop, its descriptor against a per-sample loop, the float32
oracle (oracle/sift_pyramid.py, oracle/sift_oracle.py) within every bound it derives at 3 and 4
layers per octave with few undecided items, and the known answers of the keypoint stages."""
import numpy as np
import pytest

import sift_f64 as sf
from test_multiband_f64 import _reflect101
from test_oracle_golden import (SIFT_BLOBS, _blob_scene, check_blob_keypoints, check_ramp_orientation,
                                check_rot90)


def _step_loop(plane, taps):
    t = np.asarray(taps, np.float32).astype(np.float64)
    r = len(t) // 2
    h, w = plane.shape
    x = np.asarray(plane, np.float64)
    cols = np.array([[_reflect101(c + j - r, w) for j in range(len(t))] for c in range(w)])
    rows = np.array([[_reflect101(y + j - r, h) for j in range(len(t))] for y in range(h)])
    mid = np.einsum("j,yxj->yx", t, x[:, cols])
    return np.einsum("j,yjx->yx", t, mid[rows])


@pytest.mark.parametrize("shape", [(37, 53), (1, 40), (40, 1), (2, 45), (45, 2), (3, 3), (1, 1),
                                   (3, 70)])
@pytest.mark.parametrize("ntaps", [9, 27, 33])
def test_step_f64_equals_a_direct_tap_loop(shape, ntaps):
    """Ragged planes and planes 1, 2 and 3 px on a side, where REFLECT_101 bounces more than once
    at 27 and 33 taps: SciPy's mirror mode is the kernels' border, to float64 rounding."""
    from pano360_amd import engine
    rng = np.random.default_rng(shape[0] * 97 + shape[1] + ntaps)
    sigma = (ntaps - 1) / 8.0
    taps = engine.gaussian_taps(ntaps, sigma)
    assert engine.gaussian_ksize(sigma) == ntaps
    plane = (rng.random(shape) * 255).astype(np.float32)
    np.testing.assert_allclose(sf.step_f64(plane, taps), _step_loop(plane, taps), rtol=1e-13)


def _descriptor_loop(img, kx, ky, ksize, kangle, packed):
    """calcSIFTDescriptor as one scalar loop over the window's samples, in float64."""
    import math
    octave, _ = sf.unpack_octave(packed)
    scale = 2.0 ** -octave
    px, py = int(np.rint(np.float32(kx) * np.float32(scale))), int(np.rint(np.float32(ky) * np.float32(scale)))
    ori = float(np.float32(360.0) - np.float32(kangle))
    ori = 0.0 if abs(ori - 360.0) < sf.FLT_EPSILON else ori
    scl = float(np.float32(ksize) * np.float32(scale) * np.float32(0.5))
    hw = 3.0 * scl
    radius = int(round(hw * math.sqrt(2) * 2.5)) + 2
    rows, cols = img.shape
    cos_t, sin_t = math.cos(math.radians(ori)) / hw, math.sin(math.radians(ori)) / hw
    hist = np.zeros((6, 6, 10))
    im = np.asarray(img, np.float64)
    for i in range(-radius, radius + 1):
        for j in range(-radius, radius + 1):
            c_rot, r_rot = j * cos_t - i * sin_t, j * sin_t + i * cos_t
            rbin, cbin = r_rot + 1.5, c_rot + 1.5
            r, c = py + i, px + j
            if not (-1 < rbin < 4 and -1 < cbin < 4 and 0 < r < rows - 1 and 0 < c < cols - 1):
                continue
            dx, dy = im[r, c + 1] - im[r, c - 1], im[r - 1, c] - im[r + 1, c]
            mag = math.hypot(dx, dy) * math.exp(-(c_rot ** 2 + r_rot ** 2) / 8.0)
            obin = (float(sf.fast_atan2_f64(dy, dx)) - ori) * 8 / 360.0
            r0, c0, o0 = math.floor(rbin), math.floor(cbin), math.floor(obin)
            fr, fc, fo = rbin - r0, cbin - c0, obin - o0
            for a, wa in ((0, 1 - fr), (1, fr)):
                for b, wb in ((0, 1 - fc), (1, fc)):
                    for o, wo in ((0, 1 - fo), (1, fo)):
                        hist[r0 + 1 + a, c0 + 1 + b, (o0 % 8) + o] += mag * wa * wb * wo
    hist[:, :, 0] += hist[:, :, 8]
    hist[:, :, 1] += hist[:, :, 9]
    v = hist[1:5, 1:5, :8].reshape(-1)
    v = np.minimum(v, 0.2 * np.sqrt((v * v).sum()))
    return v * 512.0 / max(np.sqrt((v * v).sum()), sf.FLT_EPSILON)


@pytest.mark.parametrize("case", [(20.3, 17.6, 6.0, 37.0, 0), (2.0, 30.5, 9.0, 359.999, 0),
                                  (63.0, 0.0, 4.0, 90.0, 0), (10.25, 12.75, 3.2, 0.0, 255),
                                  (8.0, 6.0, 30.0, 180.0, 1)])
def test_descriptor_f64_equals_a_per_sample_loop(case):
    """The vectorised descriptor against a scalar loop over the samples: windows cut by the
    border, the orientation wrap, octave -1 and a window larger than the plane."""
    rng = np.random.default_rng(7)
    img = (rng.random((32, 64)) * 255).astype(np.float32)
    x, y, size, angle, octave = case
    packed = octave | (1 << 8)
    got, delta = sf.descriptor_f64(img, x, y, size, angle, packed)
    want = _descriptor_loop(img, x, y, size, angle, packed)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9)
    assert (delta >= 0).all() and delta.max() < 0.05


def _frames():
    from scipy import ndimage
    from pano360_amd import synth
    rng = np.random.default_rng(3)
    noise = ndimage.gaussian_filter(rng.random((48, 64)), 1.5)
    noise = np.stack([((noise - noise.min()) / np.ptp(noise) * 255).astype(np.uint8)] * 3, -1)
    return {"B": synth.make_frame(3, 96, 72, "B"), "blobs": _blob_scene(SIFT_BLOBS, size=96),
            "noise": noise}


def oracle_against_f64(gauss, dog, n_layers):
    """(candidates, undecided, worst e per quantity) of the float32 oracle's refinement against
    ``refine_f64``; asserts every decided outcome and every bound."""
    import sift_oracle as so
    total = undecided = 0
    worst = {"x": 0.0, "y": 0.0, "size": 0.0, "response": 0.0}
    for o in range(len(dog)):
        stack = np.stack(dog[o])
        cands = sf.extrema(stack, n_layers)
        res = sf.refine_f64(stack, o, cands, n_layers)
        for k, (layer, r, c) in enumerate(cands):
            kp = so.adjust_local_extrema(dog[o], o, int(layer), int(r), int(c), n_layers)
            total += 1
            if not res["decided"][k]:
                undecided += 1
                continue
            assert (kp is not None) == res["kept"][k], (o, layer, r, c)
            if kp is None:
                continue
            for key in worst:
                e = abs(float(kp[key]) - res[key][k]) / res["d" + ("resp" if key == "response" else key)][k]
                worst[key] = max(worst[key], e)
                assert e <= 1.0, (key, o, layer, r, c, e)
            assert (kp["r"], kp["c"], kp["layer"]) == (res["r"][k], res["c"][k], res["layer"][k])
            mask = -1 if res["oct_decided"][k] else 0xffff
            assert kp["octave"] & mask == res["octave"][k] & mask
    return total, undecided, worst


@pytest.mark.parametrize("n_layers", [3, 4])
def test_oracle_within_every_bound_of_the_f64_restatement(n_layers):
    """Criterion 2 of the GPU judge: the float32 oracle's scale steps, refinement and descriptors
    within the bounds of sift_f64, every decided outcome the same; under 2 % of a frame's
    candidates undecided (the blob scene: a third, see below)."""
    import sift_oracle as so
    import sift_pyramid as sp
    from pano360_amd import features
    taps = [features._step_taps(s) for s in sp.sigmas(layers=n_layers)]
    for name, bgr in _frames().items():
        gauss, dog = sp.sift_pyramid(bgr, layers=n_layers)
        worst_step = 0.0
        for o in range(min(2, len(gauss))):
            for i in range(1, n_layers + 3):
                e = sf.step_error(gauss[o][i], sf.step_f64(gauss[o][i - 1], taps[i]))
                assert e.max() <= sf.step_bound(len(taps[i])), (name, o, i, e.max())
                worst_step = max(worst_step, float(e.max()) / sf.step_bound(len(taps[i])))
        total, undecided, worst = oracle_against_f64(gauss, dog, n_layers)
        assert total > 10, (name, total)
        # the blob scene's flat background holds a few candidates just above the threshold whose
        # Hessians are near singular (Newton steps of tens of pixels): rightly undecided, and a
        # third of that scene's few candidates at most; every other frame under 2 %
        assert undecided <= (total / 3 if name == "blobs" else 0.02 * total), (name, undecided, total)
        kps, des = so.detect_and_compute(gauss, dog, n_layers)
        excess = 0.0
        for k, d in zip(kps[:40], des[:40]):
            octave, layer = sf.unpack_octave(int(k["octave"]))
            v, delta = sf.descriptor_f64(gauss[octave + 1][layer], k["x"], k["y"], k["size"],
                                         k["angle"], int(k["octave"]))
            err = np.abs(d - np.clip(v, 0, 255))
            assert (err <= 0.5 + delta).all(), (name, float((err - 0.5 - delta).max()))
            excess = max(excess, float(err.max()))
        print(f"{name} layers {n_layers}: step e/E {worst_step:.3f}, refinement e/E "
              f"{ {k: round(v, 3) for k, v in worst.items()} }, undecided {undecided}/{total}, "
              f"descriptor |got - v| {excess:.3f}")



def test_f64_keypoints_pass_the_known_answers():
    """The blobs of test_oracle_golden.py found where the closed form puts them by the float64
    refinement of the oracle's scale space (decided keypoints, first-octave adjustment)."""
    import sift_pyramid as sp
    gauss, dog = sp.sift_pyramid(_blob_scene(SIFT_BLOBS))
    kps = []
    for o in range(len(dog)):
        stack = np.stack(dog[o])
        res = sf.refine_f64(stack, o, sf.extrema(stack, 3), 3)
        keep = res["kept"] & res["decided"]
        kps += [dict(x=0.5 * x, y=0.5 * y, size=0.5 * s)
                for x, y, s in zip(res["x"][keep], res["y"][keep], res["size"][keep])]
    check_blob_keypoints(kps)


def test_pivot_threshold_is_ten_flt_epsilon():
    """The oracle's solve gives up below 10 FLT_EPSILON, as sift.hip's solve3 (sift_f64 docstring):
    a pivot of 5 FLT_EPSILON is singular, one of 20 FLT_EPSILON is not."""
    import sift_oracle as so
    eps = np.float32(sf.FLT_EPSILON)
    for p, singular in ((5 * eps, True), (20 * eps, False)):
        h = np.diag([np.float32(0.5), np.float32(0.25), p]).astype(np.float32)
        sol = so._solve3(h, np.ones(3, np.float32))
        assert (sol is None) == singular
        piv = np.abs(sf.lu_pivots(h[None].astype(np.float64)))[0]
        assert (piv < sf.PIVOT_EPS).any() == singular


def _orient_loop(img, r, c, size, octv):
    """calcOrientationHist's raw histogram as one scalar loop over the window, in float64."""
    import math
    scl = float(np.float32(np.float32(size) * np.float32(0.5)) / np.float32(1 << octv))
    radius = int(np.rint(np.float32(4.5) * np.float32(scl)))
    sig = float(np.float32(1.5) * np.float32(scl))
    rows, cols = img.shape
    im = np.asarray(img, np.float64)
    hist = np.zeros(36)
    for i in range(-radius, radius + 1):
        for j in range(-radius, radius + 1):
            y, x = r + i, c + j
            if not (0 < y < rows - 1 and 0 < x < cols - 1):
                continue
            dx, dy = im[y, x + 1] - im[y, x - 1], im[y - 1, x] - im[y + 1, x]
            w = math.exp(-(i * i + j * j) / (2.0 * sig * sig))
            hist[int(np.rint(float(sf.fast_atan2_f64(dy, dx)) / 10.0)) % 36] += w * math.hypot(dx, dy)
    return hist


def _f64_detect(bgr, with_desc=False):
    """detectAndCompute with every keypoint stage in float64 (sift_f64) on the oracle's scale
    space: decided keypoints and decided peaks only, OpenCV's first-octave adjustment."""
    import sift_pyramid as sp
    gauss, dog = sp.sift_pyramid(bgr)
    kps, desc = [], []
    for o in range(len(dog)):
        stack = np.stack(dog[o])
        res = sf.refine_f64(stack, o, sf.extrema(stack, 3), 3)
        for k in np.nonzero(res["kept"] & res["decided"])[0]:
            layer = int(res["layer"][k])
            for angle, _, dec in sf.orientation_f64(gauss[o][layer], int(res["r"][k]),
                                                    int(res["c"][k]), res["size"][k], o):
                if not dec:
                    continue
                octave = (int(res["octave"][k]) & ~255) | ((o - 1) & 255)
                kp = dict(x=np.float32(0.5 * res["x"][k]), y=np.float32(0.5 * res["y"][k]),
                          size=np.float32(0.5 * res["size"][k]), angle=np.float32(angle), octave=octave)
                kps.append(kp)
                if with_desc:
                    v, _ = sf.descriptor_f64(gauss[o][layer], kp["x"], kp["y"], kp["size"], kp["angle"],
                                             octave)
                    desc.append(np.rint(np.clip(v, 0, 255)))
    return (kps, np.array(desc)) if with_desc else kps


@pytest.mark.parametrize("case", [(20, 30, 6.0, 0), (1, 1, 9.0, 0), (30, 62, 12.0, 0), (5, 9, 3.0, 1)])
def test_orientation_f64_against_a_per_sample_loop(case):
    """The vectorised orientation histogram against a scalar loop over the window (windows cut by
    the border, octave 1), and its error scales non-negative and small."""
    rng = np.random.default_rng(9)
    img = (rng.random((32, 64)) * 255).astype(np.float32)
    r, c, size, octv = case
    hist, err = sf.orientation_hist_f64(img, r, c, size, octv)
    np.testing.assert_allclose(hist, _orient_loop(img, r, c, size, octv), rtol=1e-10, atol=1e-9)
    assert (err >= 0).all()


def test_oracle_angles_within_the_f64_orientation():
    """Criterion 2 for the orientation: the float32 oracle's angles of every refined keypoint of two
    B frames and the blob scene within the bounds of orientation_f64, every decided peak present
    and every oracle angle one of the possible peaks."""
    import sift_oracle as so
    import sift_pyramid as sp
    from pano360_amd import synth
    worst, total, undecided = 0.0, 0, 0
    for bgr in (synth.make_frame(3, 96, 72, "B"), synth.make_frame(8, 80, 64, "B"),
                _blob_scene(SIFT_BLOBS, size=96)):
        gauss, dog = sp.sift_pyramid(bgr)
        for o in range(len(dog)):
            stack = np.stack(dog[o])
            res = sf.refine_f64(stack, o, sf.extrema(stack, 3), 3)
            for k in np.nonzero(res["kept"] & res["decided"])[0]:
                img = gauss[o][int(res["layer"][k])]
                r, c, size = int(res["r"][k]), int(res["c"][k]), np.float32(res["size"][k])
                got = [float(a) for a in so.orientation_angles(img, r, c, size, o)]
                peaks = sf.orientation_f64(img, r, c, size, o)
                for a, da, dec in peaks:
                    total += 1
                    if not dec:
                        undecided += 1
                        continue
                    d = [abs((g - a + 180.0) % 360.0 - 180.0) for g in got]
                    assert d and min(d) <= da, (a, da, got)
                    worst = max(worst, min(d) / da)
                for g in got:
                    assert any(abs((g - a + 180.0) % 360.0 - 180.0) <= da for a, da, _ in peaks)
    assert total > 200 and undecided <= 0.02 * total, (undecided, total)
    print(f"orientation: oracle worst e/E {worst:.3f}, undecided {undecided}/{total}")


def test_f64_keypoints_pass_the_ramp_and_quarter_turn_answers():
    """The ramp's direction and the quarter turn of test_oracle_golden.py, passed by keypoints,
    angles and descriptors made wholly in float64."""
    check_ramp_orientation(_f64_detect)
    check_rot90(_f64_detect)
