"""The MSOP kernels (csrc/msop.hip) against the NumPy model (tests/msop_model.py), stage by
stage through ``msop_detect_device(want_stages=True)``, on the three golden fixtures.

Harris response, cut lists, the ``ssc`` selections, g_x, g_y and the blurred plane are equal to
the model bit for bit.  theta is the one value the device's libm decides (``atan2f``): it must lie
within 2e-6 rad of float64 ``atan2`` of the model's float32 gradients (6 float32 ulps at pi,
OpenCL's bound for atan2, plus the final rounding).  The model is then fed the device's theta, so
the rest is determined: raw tiles and descriptors are equal bit for bit, except that a last-bit
difference of double cos / sin may move a sample across a 1/32 rounding boundary - at most 1 patch
in 1000, and then by no more than twice the fixture's recorded worst difference of that kind.
"""
import functools
import os

import numpy as np
import pytest

import msop_model as mm
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURES = ("noise", "odd", "flat")
PLANES = ("g_x", "g_y", "blurred")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(GOLDEN, f"msop_{name}.npz")) as g:
        return {k: g[k] for k in g.files}


def device_run(eng, img, max_feat):
    """(points, descs, stages) of the device as host arrays."""
    from pano360_amd import features
    frame = eng.upload_frames([img])[0]
    points, descs, stages = features.msop_detect_device(frame, max_feat, eng, want_stages=True)
    host = [{k: v.cpu().numpy() for k, v in st.items()} for st in stages]
    return points.cpu().numpy(), descs.cpu().numpy(), host


_RUNS = {}


def run(eng, name):
    """Device and model results of a fixture, computed once; the model is fed the device's theta
    (its own angles stay in ``own``)."""
    if name not in _RUNS:
        if name == "large":
            img = np.repeat(mm.smooth_noise(540, 960, 31)[..., None], 3, axis=2)
            max_feat, worst = (5000, 100, 25, 10), max(float(golden(n)["desc_worst"])
                                                        for n in FIXTURES)
        else:
            g = golden(name)
            img, max_feat = g["img"], tuple(int(v) for v in g["max_feat"])
            worst = float(g["desc_worst"])
        dev = device_run(eng, img, max_feat)
        own = mm.detect(img, max_feat, want_stages=True)[2]
        try:
            fed = mm.detect(img, max_feat, thetas_in=[st["theta"] for st in dev[2]],
                            want_stages=True)
        except (ValueError, IndexError):          # the selections differ: their test says so
            fed = None
        _RUNS[name] = {"dev": dev, "own": own, "fed": fed, "worst": worst}
    return _RUNS[name]


CASES = FIXTURES + ("large",)       # large: 540 x 960 with the default max_feat


@pytest.mark.parametrize("name", CASES)
def test_harris_response_bits(eng, name):
    r = run(eng, name)
    for lvl, (d, m) in enumerate(zip(r["dev"][2], r["own"])):
        assert d["hrs"].shape == m["hrs"].shape
        assert np.array_equal(bits(d["hrs"]), bits(m["hrs"])), f"level {lvl}"


@pytest.mark.parametrize("name", CASES)
def test_cut_lists_equal(eng, name):
    r = run(eng, name)
    for lvl, (d, m) in enumerate(zip(r["dev"][2], r["own"])):
        assert np.array_equal(d["cut"], m["cut"]), f"level {lvl}"


@pytest.mark.parametrize("name", CASES)
def test_ssc_selections_equal(eng, name):
    r = run(eng, name)
    for lvl, (d, m) in enumerate(zip(r["dev"][2], r["own"])):
        assert np.array_equal(d["sel"], m["sel"]), f"level {lvl}"
    if name == "large":
        assert len(r["own"][0]["cut"]) > 20000       # tens of thousands of points per probe


@pytest.mark.parametrize("name", CASES)
def test_gradient_and_blurred_planes_bits(eng, name):
    r = run(eng, name)
    for lvl, (d, m) in enumerate(zip(r["dev"][2], r["own"])):
        for key in PLANES:
            assert np.array_equal(bits(d[key]), bits(m[key])), f"level {lvl}: {key}"


@pytest.mark.parametrize("name", CASES)
def test_theta_within_atan2_bound(eng, name):
    r = run(eng, name)
    for lvl, (d, m) in enumerate(zip(r["dev"][2], r["own"])):
        rows, cols = m["cut"][m["sel"], 0], m["cut"][m["sel"], 1]
        want = np.arctan2(m["g_x"][rows, cols].astype(np.float64),
                          m["g_y"][rows, cols].astype(np.float64))
        err = np.abs(d["theta"].astype(np.float64) - want)
        print(f"{name} level {lvl}: worst theta error {err.max():.3g} rad")
        assert err.max() <= 2e-6


@pytest.mark.parametrize("name", CASES)
def test_tiles_and_descriptors_bits(eng, name):
    r = run(eng, name)
    assert r["fed"] is not None, "the device's points are not the model's"
    dev_descs = r["dev"][1]
    tiles = np.concatenate([st["tiles"].reshape(-1, 64) for st in r["dev"][2]])
    m_tiles = np.concatenate([st["tiles"].reshape(-1, 64) for st in r["fed"][2]])
    m_descs = r["fed"][1]
    assert tiles.shape == m_tiles.shape and dev_descs.shape == m_descs.shape
    diff_t = np.abs(tiles.astype(np.float64) - m_tiles).max(axis=1)
    diff_d = np.abs(dev_descs.astype(np.float64) - m_descs).max(axis=1)
    same = (bits(tiles) == bits(m_tiles)).all(axis=1) & (bits(dev_descs) == bits(m_descs)).all(axis=1)
    n_diff = int(np.count_nonzero(~same))
    print(f"{name}: {n_diff} of {len(same)} patches differ; worst tile difference "
          f"{diff_t.max():.4g}, descriptor {diff_d.max():.4g}; allowed {2 * r['worst']:.4g}")
    assert n_diff <= len(same) / 1000
    assert diff_d.max() <= 2 * r["worst"]
    # a patch whose tile is the model's has the model's descriptor: the normalisation is exact
    tiles_same = (bits(tiles) == bits(m_tiles)).all(axis=1)
    assert (bits(dev_descs)[tiles_same] == bits(m_descs)[tiles_same]).all()


@pytest.mark.parametrize("name", CASES)
def test_point_tuples(eng, name):
    r = run(eng, name)
    points = r["dev"][0]
    assert points.dtype == np.float64 and points.shape[1] == 4
    theta = np.concatenate([st["theta"] for st in r["dev"][2]])
    assert np.array_equal(points[:, 2], theta.astype(np.float64))
    want = np.concatenate([st["points"] for st in r["own"]])
    assert np.array_equal(points[:, [0, 1, 3]], want[:, [0, 1, 3]])


@pytest.mark.parametrize("name", FIXTURES)
def test_msop_detect_points_equal_the_reference(eng, name):
    from pano360_amd import features
    g = golden(name)
    points, descs = features.msop_detect(g["img"], tuple(int(v) for v in g["max_feat"]))
    assert points.dtype == np.float64 and descs.dtype == np.float32
    assert descs.shape == (len(points), 64)
    assert np.array_equal(points[:, [0, 1, 3]], g["points"][:, [0, 1, 3]])
    assert np.abs(points[:, 2] - g["points"][:, 2]).max() <= 2e-6


@pytest.mark.parametrize("shape", ((37, 53), (3, 4), (1, 70), (130, 9)))
@pytest.mark.parametrize("ksize", (1, 3, 5, 11, 15))
def test_smooth_equals_the_separable_filter_bits(eng, shape, ksize):
    """``pano_msop_smooth`` directly: every aperture path (5 and 11 are compiled for their tap
    count, the others share the general kernel), planes smaller than the radius (several
    reflections) and wider than a block, against the oracle's separable filter bit for bit."""
    import torch
    import cv2_shim
    from pano360_amd import _lib, engine
    plane = (np.random.default_rng(3).random(shape) * 255 - 100).astype(np.float32)
    taps = np.ascontiguousarray(engine.gaussian_taps(ksize, 0.3 * ksize + 0.5))
    src = torch.from_numpy(plane).to(eng.device)
    tmp, dst = torch.empty_like(src), torch.empty_like(src)
    _lib.check(eng.lib.pano_msop_smooth(eng.ctx(), engine._ptr(src), shape[0], shape[1],
                                        taps.ctypes.data, ksize, engine._ptr(tmp),
                                        engine._ptr(dst)), "pano_msop_smooth")
    want = cv2_shim.sep_filter_symm(plane, taps)
    assert np.array_equal(bits(dst.cpu().numpy()), bits(want))


# ------------------------------------------------------------------ ssc, direct calls
def random_points(h, w, n, seed):
    flat = np.random.default_rng(seed).choice(h * w, n, replace=False)
    return np.stack([flat // w, flat % w], axis=1)


def found_set(seed):
    """The draw tests/test_msop_host.py found its `low > high` sets with."""
    rng = np.random.default_rng(seed)
    n, n_points = int(rng.integers(20, 400)), int(rng.integers(3, 60))
    flat = rng.choice(64 * 80, n, replace=False)
    return np.stack([flat // 80, flat % 80], axis=1), (64, 80), n_points


def ssc_case(name):
    if name == "3000-of-200":
        return random_points(192, 256, 3000, 5), (192, 256), 200
    if name == "40-of-50":                       # fewer points than asked: cgr < 1
        return random_points(192, 256, 40, 5), (192, 256), 50
    if name == "low-high":                       # ends through low > high after three probes
        return found_set(4)
    if name == "past-onchip":                    # a grid of 581 746 cells: past the LDS bitmap
        return found_set(23)
    raise KeyError(name)


@pytest.mark.parametrize("path", ("auto", "onchip", "global"))
@pytest.mark.parametrize("name", ("3000-of-200", "40-of-50", "low-high", "past-onchip"))
def test_ssc_equals_the_model(eng, name, path):
    from pano360_amd import _lib, features
    pts, im_size, n_points = ssc_case(name)
    want = [tuple(p) for p in mm.ssc(pts, im_size, n_points)]
    if name == "past-onchip" and path == "onchip":
        with pytest.raises(_lib.PanoError):
            features.ssc(pts, im_size, n_points, path=path)
        return
    got = features.ssc(pts, im_size, n_points, path=path)
    assert [tuple(int(v) for v in p) for p in got] == want
    if name == "40-of-50":
        assert len(got) == 40


def test_value_errors(eng):
    from pano360_amd import features
    with pytest.raises(ValueError):
        features.ssc(random_points(32, 32, 50, 1), (32, 32), 1)
    with pytest.raises(ValueError):
        features.ssc(np.array([[40, 3]]), (32, 32), 5)           # outside im_size
    with pytest.raises(ValueError):
        features.msop_detect(np.full((5, 5, 3), 90, np.uint8), (2,))


# ------------------------------------------------------------------ end to end
def test_msop_detector_registers_a_shifted_pair(eng):
    """Two crops of one texture, offset by (dy, dx) = (16, 72): ``matching`` with the MSOP detector
    must register them, and its homography must carry the corners of the first crop to within a
    pixel of the pure translation (the keypoints are centred on equal-sized images, so the
    translation is the same in centred coordinates)."""
    from pano360_amd import features
    a, b = mm.shifted_pair()
    detect = features.msop_detector((200, 50, 12, 6))
    kp_, des = detect(a)
    assert des.shape == (len(kp_), 64) and des.dtype == np.float32
    m_points = mm.detect(a, (200, 50, 12, 6))[0]
    assert [k.pt for k in kp_] == [(float(p[1]), float(p[0])) for p in m_points]
    assert np.abs(np.array([k.size for k in kp_]) - m_points[:, 2]).max() <= 2e-6   # size: theta
    kpts, matches = features.matching([a, b], detect=detect)
    table = matches[()]
    assert 1 in table[0] and 0 in table[1], "the pair did not register"
    match, hom = table[0][1]
    assert len(match) >= features.N_MIN_MATCH
    corners = np.array([[0, 0], [255, 0], [255, 191], [0, 191]], np.float64) - [128, 96]
    mapped = np.concatenate([corners, np.ones((4, 1))], axis=1) @ hom.T
    mapped = mapped[:, :2] / mapped[:, 2:]
    err = np.abs(mapped - (corners + [-72, -16])).max()
    print(f"{len(match)} inliers, worst corner error {err:.3f} px")
    assert err <= 1.0


def test_determinism_and_after_sift(eng):
    from pano360_amd import features
    g = golden("noise")
    max_feat = tuple(int(v) for v in g["max_feat"])
    first = features.msop_detect(g["img"], max_feat)
    second = features.msop_detect(g["img"], max_feat)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    features.sift_detector(eng)(g["img"])
    third = features.msop_detect(g["img"], max_feat)
    assert first[0].tobytes() == third[0].tobytes() and first[1].tobytes() == third[1].tobytes()
