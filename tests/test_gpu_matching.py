"""GPU: pano_hom_ransac - the kernels against the NumPy model of their contract
(tests/ransac_model.py: every hypothesis's score bit for bit), batch independence and
determinism, a known answer through ``find_homography``, and ``matching`` end to end on a rig
rendered from one panorama.  The tests of the kernels enter at ``find_homographies_device``, after
the ratio test and the packing: pano_match_pack runs here only inside ``matching``, and is tested
on its own, against the model of its contract, in tests/test_gpu_match_pack.py.  Every frame here
is 1280 x 720, detected on an engine of this module's own: frame sizes never mix in one engine."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_model as rm  # noqa: E402

pytestmark = pytest.mark.gpu

ITERS = 1000                 # not a multiple of the kernel's 256 hypotheses per block
THRESH = 3.0
SEED = 12345


def _hom(rng, w=1280, h=720, spread=0.1):
    from pano360_amd.bundle_adj import intrinsics, rotation_to_mat
    K = intrinsics(w / (2 * np.tan(np.deg2rad(30))))
    H = K @ rotation_to_mat(rng.normal(0.0, spread, 3)) @ np.linalg.inv(K)
    return H / H[2, 2]


def _pair(rng, n, outliers, noise=0.5, w=1280, h=720):
    """(pts float32 [n][4], true inlier mask, H): noise of sigma `noise` clipped at 2 px per
    coordinate, outliers at least 20 px from the truth."""
    H = _hom(rng)
    src = rng.uniform([-w / 2, -h / 2], [w / 2, h / 2], (n, 2))
    dst = rm.project(H, src) + np.clip(rng.normal(0.0, noise, (n, 2)), -2.0, 2.0)
    bad = rng.random(n) < outliers
    k = int(bad.sum())
    ang = rng.uniform(0, 2 * np.pi, k)
    dst[bad] = rm.project(H, src[bad]) + rng.uniform(20.0, 300.0, (k, 1)) * np.c_[np.cos(ang), np.sin(ang)]
    return np.c_[src, dst].astype(np.float32), ~bad, H


def _batch():
    rng = np.random.default_rng(2024)
    sets = [_pair(rng, 3, 0.0)[0], _pair(rng, 4, 0.0)[0], _pair(rng, 5, 0.2)[0],
            _pair(rng, 8, 0.25)[0], _pair(rng, 200, 0.0)[0], _pair(rng, 200, 0.9)[0],
            _pair(rng, 5000, 0.3)[0], _pair(rng, 20000, 0.6)[0], _pair(rng, 1000, 0.5, 1.0)[0],
            _pair(rng, 300, 0.8)[0]]
    line = np.zeros((500, 4), np.float32)                       # fully collinear
    t = rng.integers(-300, 300, 500)                            # (exact in float32 and f64)
    line[:, 0], line[:, 1], line[:, 2], line[:, 3] = t, 2 * t + 3, 3 * t + 1, 5 - t
    sets.append(line)
    same = np.repeat(rng.uniform(-200, 200, (3, 4)), 40, axis=0).astype(np.float32)   # 3 places
    sets.append(same)
    return sets


def _run(sets, order=None, scores=True):
    """Pack the sets into one buffer (in `order`, so offsets are not monotonic) and run one
    pano_hom_ransac; host results in the sets' order."""
    import torch
    from pano360_amd import features
    order = list(range(len(sets))) if order is None else order
    offsets = np.zeros(len(sets), np.int32)
    rows, at = [], 0
    for k in order:
        offsets[k] = at
        rows.append(sets[k])
        at += len(sets[k])
    pts = torch.from_numpy(np.concatenate(rows)).cuda()
    counts = torch.tensor([len(s) for s in sets], dtype=torch.int32)
    out = features.find_homographies_device(pts, torch.from_numpy(offsets), counts, ITERS, THRESH,
                                            SEED, want_scores=scores)
    host = [t.cpu().numpy() for t in out]
    masks = [host[1][offsets[k]:offsets[k] + len(sets[k])] for k in range(len(sets))]
    return host[0], masks, host[2], (host[3] if scores else None)


@pytest.fixture(scope="module")
def batch():
    sets = _batch()
    return sets, [rm.ransac(s, SEED, ITERS, THRESH) for s in sets]


def test_kernel_equals_model(batch):
    sets, model = batch
    hom, masks, n_inl, scores = _run(sets, order=list(range(len(sets)))[::-1])
    failed = 0
    for k, (pts, (H, mask, n, best, sc)) in enumerate(zip(sets, model)):
        assert np.array_equal(scores[k], sc), (k, np.nonzero(scores[k] != sc)[0][:10])
        assert n_inl[k] == n, k
        assert np.array_equal(masks[k], mask), k
        if H is None:
            failed += 1
            assert not hom[k].any() and n_inl[k] == 0 and not masks[k].any(), k
            continue
        assert int(np.argmax(scores[k])) == best
        assert hom[k][2, 2] == 1.0
        inl = pts[mask != 0].astype(np.float64)
        err = np.abs(rm.project(hom[k], inl[:, :2]) - rm.project(H, inl[:, :2])).max()
        assert err < 1e-5, (k, err)
    assert failed >= 3                      # 3 rows, the collinear set, the coincident set


def test_batch_independence_and_determinism(batch):
    sets, _ = batch
    hom, masks, n_inl, scores = _run(sets)
    hom2, masks2, n_inl2, scores2 = _run(sets, order=list(range(len(sets)))[::-1])
    assert np.array_equal(hom, hom2) and np.array_equal(n_inl, n_inl2)
    assert np.array_equal(scores, scores2) and all(np.array_equal(a, b) for a, b in zip(masks, masks2))
    for k in (1, 4, 6, 7, 10):
        h1, m1, n1, s1 = _run([sets[k]], scores=False)
        assert np.array_equal(h1[0], hom[k]) and n1[0] == n_inl[k]
        assert np.array_equal(m1[0], masks[k]) and s1 is None


def test_find_homography_known_answer():
    """The estimate's own error decides the size: with 750 inliers at sigma 0.5 px the DLT over
    exactly the true inliers is already 0.11 - 0.17 px off at the frame's corners (measured), so
    the 0.1 px bound takes 20 000 correspondences (0.02 - 0.03 px)."""
    from pano360_amd import features
    rng = np.random.default_rng(77)
    grid = np.stack(np.meshgrid(np.linspace(-640, 640, 33), np.linspace(-360, 360, 19)), -1).reshape(-1, 2)
    for trial in range(3):
        pts, good, H = _pair(rng, 20000, 0.25)
        src, dst = pts[:, :2].reshape(-1, 1, 2), pts[:, 2:].reshape(-1, 1, 2)
        Hf, mask = features.find_homography(src, dst, features.RANSAC, 3.0)
        assert Hf.shape == (3, 3) and Hf.dtype == np.float64 and Hf[2, 2] == 1.0
        assert mask.shape == (20000, 1) and mask.dtype == np.uint8
        assert np.array_equal(mask[:, 0].astype(bool), good), trial
        # the refit is the normalised DLT over the true inliers
        p = pts.astype(np.float64)
        dlt = rm.refit(p[good, :2], p[good, 2:])
        assert np.abs(rm.project(Hf, grid) - rm.project(dlt, grid)).max() < 1e-5
        err = np.abs(rm.project(Hf, grid) - rm.project(H, grid)).max()
        print(f"known answer, trial {trial}: max reprojection error {err:.4f} px over the frame")
        assert err < 0.1, (trial, err)
    with pytest.raises(ValueError):
        features.find_homography(src, dst, 0)
    assert features.find_homography(src[:3], dst[:3]) == (None, None)


# ------------------------------------------------------------------ a rendered rig
W, H_, N_FRAMES = 1280, 720, 6


@pytest.fixture(scope="module")
def rig():
    """6 frames of 1280 x 720 on a jittered yaw rig 30 degrees apart (hfov 60: half of each
    frame overlaps the next), rendered from one textured panorama; detected on an engine of this
    module's own."""
    from pano360_amd import engine, features, synth
    pano = synth.make_frame(7, 4096, 2048, "B")
    rots, intrs = synth.make_cameras(N_FRAMES, W, H_, step_deg=30.0, jitter=0.01, seed=3)
    eng = engine.Engine()
    frames = synth.render_rig(pano, rots, intrs, W, H_, eng.device)
    detect = features.sift_detector(eng)
    dets = [detect(f) for f in frames]
    return frames, rots, intrs, dets


def _replay(dets):
    it = iter(dets)
    return lambda img: next(it)


def test_matching_end_to_end_on_a_rendered_rig(rig):
    from pano360_amd import features
    frames, rots, intrs, dets = rig
    kpts, matches = features.matching(frames, detect=_replay(dets))
    assert kpts.shape == (N_FRAMES,) and kpts.dtype == object
    assert all(k.dtype == np.float32 and k.shape == (len(d[0]), 2) for k, d in zip(kpts, dets))
    m = matches.item()
    gx, gy = np.meshgrid(np.linspace(-W / 2, W / 2, 41), np.linspace(-H_ / 2, H_ / 2, 23))
    grid = np.c_[gx.ravel(), gy.ravel()]
    for i in range(N_FRAMES - 1):
        j = i + 1
        assert j in m[i], (i, j)
        match, hom = m[i][j]
        true = intrs[j] @ rots[j] @ rots[i].T @ np.linalg.inv(intrs[i])
        # the overlap: grid points of frame i that land inside frame j
        q = rm.project(true, grid)
        inside = (np.abs(q[:, 0]) < W / 2) & (np.abs(q[:, 1]) < H_ / 2)
        err = np.abs(rm.project(hom, grid[inside]) - q[inside]).max()
        print(f"pair {i}-{j}: {len(match)} inliers, max error over the overlap {err:.3f} px")
        # measured on the first run: 1175 - 1281 inliers, 0.090 - 0.120 px
        assert len(match) >= 300 and err < 0.5, (i, j, len(match), err)
        rev_m, rev_h = m[j][i]
        want_m, want_h = features._reverse(match, hom)
        assert np.array_equal(rev_m, want_m) and np.array_equal(rev_h, want_h)
        # the inlier pairs are keypoints that really correspond
        a, b = kpts[i][match[:, 0]].astype(np.float64), kpts[j][match[:, 1]].astype(np.float64)
        assert np.median(np.hypot(*(rm.project(true, a) - b).T)) < 1.0


def test_batched_matching_equals_one_pair_at_a_time(rig):
    from pano360_amd import features
    frames, _, _, dets = rig
    kpts, matches = features.matching(frames, detect=_replay(dets))
    m = matches.item()
    descs = [d[1] for d in dets]
    for i in range(N_FRAMES):
        for j in range(i + 1, N_FRAMES):
            match, hom = features._match_hom(kpts[i], kpts[j], descs[i], descs[j])
            if hom is None:
                assert j not in m.get(i, {}), (i, j)
                continue
            got_m, got_h = m[i][j]
            assert np.array_equal(got_m, match) and got_m.dtype == np.int32, (i, j)
            assert np.array_equal(got_h, hom), (i, j)
