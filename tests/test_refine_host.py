"""Host: the refinement's contract in NumPy (tests/refine_model.py) and the loop of
``bundle_adj.refine`` on the model's sums - no GPU.  The Jacobian against central differences, the
Newton inverse against the forward model, the loop on a clean and a noisy ring of
tests/refine_cases.py (the bounds are what this model reached on the CPU, times 10 or 2 as said,
each measured value beside its bound), ``lens_models`` against ``LensModel.project``, the command
line's new flags."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refine_cases as rc  # noqa: E402
import refine_model as rm  # noqa: E402

from pano360_amd import bundle_adj as ba  # noqa: E402
from pano360_amd import lens  # noqa: E402


# ------------------------------------------------------------------ the Jacobian
def _pair(case, p):
    a, b, first, count = case["table"][p].tolist()
    cams = case["cams"]
    return (cams[a, :3].copy(), cams[a, 3:].reshape(3, 3), cams[b, :3].copy(),
            cams[b, 3:].reshape(3, 3), case["rows"][first:first + count])


def test_jacobian_is_the_derivative():
    """The analytic J against central differences of the model's residual at step h = 1e-6, over
    the 600 matches of the forged pair (random points, one exactly at camera b's principal point,
    k = (-0.08, 0.01)).

    Tolerance.  Rounding: e = f (u - pi) with f <= 900 and |u|, |pi| <= 1 carries an absolute
    error of about 8 roundings (Newton's last step, s d, the two rotations' sums, the division,
    the difference) x 2^-53 x 900 = 8e-13; the central difference divides two of them by 2 h:
    8e-13 / 1e-6 = 8e-7.  Truncation: h^2 / 6 |e'''|; the third derivative by an angle is at most
    about 10 f (tan's, at 35 degrees off axis), by f or k far less: 1e-12 / 6 x 9000 = 1.5e-9.
    Bound: 1e-6 absolute (the truncation's share is within its slack).  Measured: 3.0e-7."""
    case = rc.forged_sums()
    ca, Ra, cb, Rb, rows = _pair(case, 7)
    k = np.array(rc.SUM_K)
    J, e, valid = rm.jacobian(ca, Ra, cb, Rb, rows, k)
    assert valid.sum() == 599 and valid[7] and not valid[11]
    assert np.hypot(*(rows[7, 0:2] - cb[1:3])) == 0.0
    h = 1e-6

    def res(step):
        ca2, cb2 = ca.copy(), cb.copy()
        cb2[0] += step[0]
        ca2[0] += step[4]
        return rm.residual(ca2, rm.rodrigues(step[5:8]) @ Ra, cb2, rm.rodrigues(step[1:4]) @ Rb,
                           rows, k + step[8:10])[0]
    worst = 0.0
    for c in range(10):
        step = np.zeros(10)
        step[c] = h
        fd = (res(step) - res(-step)) / (2 * h)
        worst = max(worst, float(np.max(np.abs(fd - J[:, :, c])[valid])))
        assert np.max(np.abs(J[:, :, c])[valid]) > 0.5      # no column is trivially zero
    print(f"largest |J - central difference|: {worst:.3e}")
    assert worst <= 1e-6


def test_newton_inverse():
    """forward(undist(p)) = p within 4 ulp of |p| (the forward model is three roundings on top of
    the solution's; measured: 2.5 ulp) wherever |k1| rd^2 <= 0.3 for k1 > 0.  For k1 < 0 the
    forward profile r (1 + k1 r^2) folds back at r = 1 / sqrt(3 |k1|), where it reaches
    |k1| rd^2 = 4 / 27 = 0.148: beyond that no r exists, and the matches there are invalid (h'
    <= 0), which is asserted; up to 0.148 the ten steps reach the same 4 ulp (measured: 2.0)."""
    rng = np.random.default_rng(3)
    n = 20000
    for k1 in (0.08, 0.3, -0.08, -0.3):
        limit = 0.3 if k1 > 0 else 0.148
        rd_max = np.sqrt(limit / abs(k1))
        ang = rng.uniform(0, 2 * np.pi, n)
        rd = np.sqrt(rng.uniform(0, 1, n)) * rd_max
        rd[:100] = rd_max
        rd[100] = 0.0
        p = np.c_[rd * np.cos(ang), rd * np.sin(ang)]
        _, u, _, _, _, ok = rm.undist((1.0, 0.0, 0.0), p, (k1, 0.0))
        assert ok.all()
        size = np.maximum(np.max(np.abs(p), axis=1), 1e-300)[:, None]
        err = np.abs(rm.forward(u, (k1, 0.0)) - p) / size
        print(f"k1 {k1}: {np.max(err) / 2 ** -52:.2f} ulp")
        assert np.max(err) <= 4 * 2.0 ** -52
        if k1 < 0:
            far = np.c_[np.sqrt(np.linspace(0.16, 0.3, 50) / abs(k1)), np.zeros(50)]
            assert not rm.undist((1.0, 0.0, 0.0), far, (k1, 0.0))[5].any()


# ------------------------------------------------------------------ the loop
def _refined(kind, lens_terms):
    """bundle_adj.refine's own loop on the model's sums."""
    case = rc.ring(kind)
    with rc.on_model_sums():
        return ba.refine(case["cameras"], case["matches"], case["index"], lens_terms=lens_terms,
                         huber=rc.DELTA)


def _errors(case, res):
    f = np.array([c.intr[0, 0] for c in res.cameras])
    R = np.stack([c.rot for c in res.cameras])
    return (float(np.max(np.abs(f - case["focal"]))), abs(res.k[0] - rc.K_TRUE[0]),
            rm.rotation_distance(R, case["rots"]))


def test_loop_equals_the_model():
    """The product's loop (its assembly by index maps) and the model's (the full system times a
    0 / 1 matrix), both on the model's sums: the same decisions and the same result up to the
    rounding of two assemblies (measured: f 1.2e-13 px, rotations 3.4e-16, k 0)."""
    case = rc.ring("noisy")
    before = [(c.intr.copy(), c.rot.copy()) for c in case["cameras"]]
    res, want = _refined("noisy", 1), rc.solved("noisy", 1)
    assert [h[2] for h in res.history] == [h[2] for h in want["history"]]
    assert np.allclose([h[0] for h in res.history], [h[0] for h in want["history"]], rtol=1e-12)
    f = np.array([c.intr[0, 0] for c in res.cameras])
    assert np.max(np.abs(f - want["f"])) <= 1e-11
    assert np.max(np.abs(np.stack([c.rot for c in res.cameras]) - want["R"])) <= 1e-13
    assert np.max(np.abs(np.array(res.k) - want["k"])) <= 1e-13
    assert res.n_invalid == want["n_invalid"] == 0
    assert res.inlier_share == want["inlier_share"]
    # new records; the input is as it was
    assert all(c is not o for c, o in zip(res.cameras, case["cameras"]))
    for cam, (intr, rot) in zip(case["cameras"], before):
        assert np.array_equal(cam.intr, intr) and np.array_equal(cam.rot, rot)


def test_clean_ring():
    """No noise, no outliers, k1 = -0.08, from the walk's cameras (focal lengths 971 .. 996 for the
    true 880.9, principal points up to 11 px off), lens_terms = 1.  The exact cameras are a
    minimum of cost 0, and the loop reaches it to rounding.  Measured on the model's own loop
    (``refine``'s loop on the model's sums, which is what runs here, measured 1.7e-13 px, 0,
    2.8e-16 and 2.6e-16) -> bound (x 10):
      inlier RMS     1.6e-13 px -> 1.6e-12
      focal          below one ulp of f (1.1e-13 px; the measured difference was 0) -> 1.2e-12 px
      k1             3.1e-16    -> 3.1e-15
      rotations      3.0e-16 rad -> 3.0e-15
    and every match ends within the threshold."""
    case = rc.ring("clean")
    res = _refined("clean", 1)
    f_err, k_err, r_err = _errors(case, res)
    print(f"rms {res.rms_before:.4f} -> {res.rms_after:.3e}, f {f_err:.3e}, k1 {k_err:.3e}, "
          f"rotations {r_err:.3e}, share {res.inlier_share}")
    assert res.rms_after <= 1.6e-12
    assert f_err <= 1.2e-12
    assert k_err <= 3.1e-15
    assert r_err <= 3.0e-15
    assert res.inlier_share == 1.0 and res.n_invalid == 0
    assert res.k[1] == 0.0
    for cam in res.cameras:
        assert cam.intr[0, 2] == 0 and cam.intr[1, 2] == 0
        assert np.allclose(cam.rot @ cam.rot.T, np.eye(3), atol=1e-14)


def test_noisy_ring():
    """Noise 0.5 px, 3 % outliers, 200 matches per pair, from the walk's cameras (focal lengths
    822 .. 1056 for the true 880.9, principal points up to 283 px off).  Measured -> bound (x 2):
      lens_terms = 1: inlier RMS 2.2664 -> 1.0343 px (bound 2.07), k1 error 8.58e-3 (1.72e-2),
                      focal error 2.22 px (4.44), rotations 9.3e-4 rad (1.9e-3), share 0.9619
      lens_terms = 0: inlier RMS 2.0572 px, k1 error 0.08 (k stays 0), share 0.2525"""
    case = rc.ring("noisy")
    res0, res1 = _refined("noisy", 0), _refined("noisy", 1)
    f_err, k_err, r_err = _errors(case, res1)
    print(f"lens 1: rms {res1.rms_before:.4f} -> {res1.rms_after:.4f}, f {f_err:.4f}, "
          f"k1 {k_err:.3e}, rotations {r_err:.3e}, share {res1.inlier_share}")
    print(f"lens 0: rms {res0.rms_before:.4f} -> {res0.rms_after:.4f}, share {res0.inlier_share}")
    assert res1.rms_after < res1.rms_before
    for res in (res0, res1):
        taken = [cost for cost, _, keep in res.history if keep]
        assert taken and all(x > y for x, y in zip(taken, taken[1:]))
        # (a candidate that is not taken is one whose cost did not fall)
        best = np.minimum.accumulate([np.inf] + taken)
        at = 0
        for cost, lam, keep in res.history:
            at += keep
            assert keep or not cost < best[at]
    assert k_err < abs(res0.k[0] - rc.K_TRUE[0]) == 0.08
    assert res1.rms_after < res0.rms_after
    assert res1.rms_after <= 2.07 and k_err <= 1.72e-2 and f_err <= 4.44 and r_err <= 1.9e-3
    assert res1.inlier_share > res0.inlier_share


def test_arguments():
    case = rc.ring("clean")
    cams, matches = case["cameras"], case["matches"]
    with rc.on_model_sums():
        with pytest.raises(ValueError, match="index"):
            ba.refine(cams[:5], matches)
        with pytest.raises(ValueError, match="index"):
            ba.refine(cams, matches, [0, 1, 2])
        with pytest.raises(ValueError, match="lens_terms"):
            ba.refine(cams, matches, lens_terms=3)
        with pytest.raises(ValueError, match="huber"):
            ba.refine(cams, matches, huber=0.0)
        # a subset of the cameras by index: only the pairs between them are used
        sub = ba.refine([cams[2], cams[3], cams[4]], matches, [2, 3, 4], lens_terms=0, max_iter=3)
    assert len(sub.cameras) == 3 and len(sub.history) <= 3
    sys.path.insert(0, os.path.dirname(HERE))
    import bundle_adj
    assert bundle_adj.refine is ba.refine and bundle_adj.Refinement is ba.Refinement
    assert "3.0" in ba.refine.__doc__ and "find_homographies_device" in ba.refine.__doc__
    import inspect
    assert str(inspect.signature(ba.refine)) == (
        "(cameras, matches, index=None, *, lens_terms=0, shared_focal=None, huber=3.0, "
        "max_iter=100)")


def test_gauge_is_the_first_camera_with_a_match():
    """A first camera without matches (an ``index`` subset whose image 0 has no pair among them)
    must not be the gauge: the first camera that has a match keeps its rotation, and the system
    has no free rotation left (the loop converges as on the whole ring)."""
    case = rc.ring("clean")
    cams, matches = case["cameras"], case["matches"]
    order = [0, 2, 3, 4]                     # image 0 pairs with 1 and 7 only
    pairs = ba._refine_pairs(matches, order)
    red, size = ba._refine_map(4, pairs, 1, True)
    assert np.all(red[0:4] == -1)                                   # camera 0: nothing estimated
    assert red[4] == 0 and np.all(red[5:8] == -1)                   # camera 1: f, and the gauge
    assert np.all(red[9:12] >= 0) and np.all(red[13:16] >= 0) and size == 1 + 6 + 1
    T = rm.reduction(4, rm.table_of(pairs)[1], 1, True)
    assert T.shape == (18, size) and np.array_equal((T.sum(axis=1) > 0), red >= 0)
    with rc.on_model_sums():
        res = ba.refine([cams[i] for i in order], matches, order, lens_terms=1)
    start = rm.centred(*[np.array(v) for v in (
        [cams[i].intr[0, 0] for i in order],
        [[cams[i].intr[0, 2], cams[i].intr[1, 2]] for i in order],
        [cams[i].rot for i in order])])[2]
    assert np.array_equal(res.cameras[0].rot, start[0])
    assert np.array_equal(res.cameras[1].rot, start[1])
    assert not np.array_equal(res.cameras[2].rot, start[2])
    assert res.inlier_share == 1.0 and res.rms_after < 1e-9


def test_pairs_are_every_unordered_pair_once():
    """Both directions of the dict, the upper one alone or the lower one alone give the same
    pair table: (a, b) = (camera of j, camera of i) for i < j, rows (x_i, y_i, x_j, y_j); images
    without a camera drop out."""
    matches = rc.ring("clean")["matches"]
    index = [0, 1, 2, 3, 5, 6, 7]                       # image 4 has no camera
    want = rm.pairs_of(matches, index)
    assert len(want) == 6 and max(max(a, b) for a, b, _ in want) == 6      # of the ring's 8
    upper = {i: {j: v for j, v in row.items() if i < j} for i, row in matches.items()}
    lower = {i: {j: v for j, v in row.items() if i > j} for i, row in matches.items()}
    for given in (matches, upper, lower):
        got = ba._refine_pairs(given, index)
        assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in want]
        assert all(np.array_equal(g[2], w[2]) for g, w in zip(got, want))


def test_lens_models_reproduce_the_forward_model():
    """``lens_models`` forged from a known k: where ``LensModel.project`` puts every border pixel
    of the corrected frame is where the contract's forward model puts it."""
    k = (-0.08, 0.01)
    cams = [ba.Image(None, np.eye(3), ba.intrinsics(881.0, (3.5, -2.25))),
            ba.Image(None, np.eye(3), ba.intrinsics(640.25))]
    res = ba.Refinement(cams, k, [], 0.0, 0.0, 1.0, 0)
    sizes = [(1280, 720), (161, 90)]
    models = res.lens_models(sizes)
    assert len(res.lens_models((1280, 720))) == 2
    for cam, model, (w, h) in zip(cams, models, sizes):
        f, px, py = cam.intr[0, 0], cam.intr[0, 2], cam.intr[1, 2]
        assert (model.kind, model.size, model.k) == ("brown", (w, h), (k[0], k[1], 0, 0, 0))
        assert (model.fx, model.fy, model.cx, model.cy) == (f, f, w / 2 + px, h / 2 + py)
        u, v = lens._border(w, h)
        f_new = 0.9 * f
        want = rm.forward(np.c_[(u - w / 2) / f_new, (v - h / 2) / f_new], k) * f \
            + [w / 2 + px, h / 2 + py]
        got = np.stack(model.project(u, v, f_new), axis=1)
        assert np.max(np.abs(got - want)) <= 1e-10          # pixels: a few ulp of 1280
        # and the contract's undist takes those positions back to the corrected frame's pixels
        _, und, _, _, _, ok = rm.undist((f, px, py), got - [w / 2, h / 2], k)
        assert ok.all()
        assert np.max(np.abs(und * f_new - np.c_[u - w / 2, v - h / 2])) <= 1e-9


def test_command_line():
    from pano360_amd import stitcher
    args = stitcher.parse_args(["DIR"])
    assert stitcher.refine_of(args) == (False, None)
    assert not hasattr(args, "refine") and not hasattr(args, "refine_lens")
    assert stitcher.refine_of(stitcher.parse_args(["DIR", "--refine"])) == (True, None)
    args = stitcher.parse_args(["DIR", "--refine-lens", "2"])
    assert stitcher.refine_of(args) == (True, 2) and args.refine is True
    assert stitcher.refine_of(stitcher.parse_args(["DIR", "--refine", "--refine-lens", "1"])) \
        == (True, 1)
    # no cache name changes
    assert stitcher.cache_name(args) == stitcher.cache_name(stitcher.parse_args(["DIR"]))
    for bad in (["--refine-lens", "1", "--lens", "rig.json"], ["--refine-lens", "3"],
                ["--refine-lens"]):
        with pytest.raises(SystemExit):
            stitcher.parse_args(["DIR"] + bad)


def test_abi():
    from pano360_amd import _lib
    assert "pano_ba_refine" in _lib.EXPORTS and _lib.BA_REFINE_TERMS == rm.TERMS == ba.REFINE_TERMS


def test_command_line_discards_a_refinement_that_lost_the_matches(tmp_path, monkeypatch, caplog):
    """``--refine-lens`` after a refinement that ends with fewer than half of the matches within
    the threshold: a warning, and the cameras and frames as they were - no frame is bent by a
    distortion fitted from a collapse."""
    from pano360_amd import stitcher
    case = rc.ring("clean")
    kpts = np.empty(8, object)
    for i in range(8):
        kpts[i] = np.zeros((1, 2))
    np.savez(tmp_path / "matches_X.npz", kpts=kpts, matches={0: {1: (np.zeros((1, 2), int),
                                                                   np.eye(3))}})
    monkeypatch.chdir(tmp_path)
    regions = list(case["cameras"])
    calls = []

    def refine(cameras, matches, index, lens_terms=0):
        calls.append((len(cameras), index, lens_terms))
        return ba.Refinement([ba.Image(None, np.eye(3), ba.intrinsics(5.0)) for _ in cameras],
                             (148.0, 0.0), [], float("nan"), 1.9, share, 0)

    def undistort(*args, **kw):
        raise AssertionError("frames corrected by a discarded fit")
    monkeypatch.setattr(stitcher._ba, "refine", refine)
    monkeypatch.setattr(stitcher._lens, "undistort_device", undistort)
    share = 0.23
    with caplog.at_level("WARNING"):
        out = stitcher._refine(regions, "X", None, 1)
    assert out is regions and calls == [(8, list(range(8)), 1)]
    assert "discarded" in caplog.text and "0.23" in caplog.text
    share = 0.5                                     # at the limit the refinement is used
    assert stitcher._refine(regions, "X", None, 0)[0].intr[0, 0] == 5.0
    # a missing match file, and a cache whose cameras cannot be numbered
    with pytest.raises(SystemExit, match="matches_Y.npz"):
        stitcher._refine(regions, "Y", None, 1)
    with pytest.raises(SystemExit, match="--register"):
        stitcher._refine(regions[:5], "X", None, 1)
