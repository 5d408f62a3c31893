"""CPU: the NumPy model of pano_match_pack and pano_hom_ransac (tests/ransac_model.py) on known
answers, the host ratio test of ``flann_matching`` on forged boundary distances, the
sampler's and the degeneracy test's contract, ``_reverse`` and the ``matches_<name>.npz`` layout
the reference's stitcher loads (stitcher.py:423-428, ``idx_to_keypoints``).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_model as rm  # noqa: E402


def _homography(rng, w=640, h=480):
    """A K R K^-1 homography of a small rotation (centred pixel coordinates)."""
    from pano360_amd.bundle_adj import intrinsics, rotation_to_mat
    K = intrinsics(w / (2 * np.tan(np.deg2rad(30))))
    R = rotation_to_mat(rng.normal(0.0, 0.08, 3))
    H = K @ R @ np.linalg.inv(K)
    return H / H[2, 2]


def _pairs(rng, H, n, outliers, w=640, h=480, noise=0.0):
    src = rng.uniform([-w / 2, -h / 2], [w / 2, h / 2], (n, 2))
    dst = rm.project(H, src) + rng.normal(0.0, noise, (n, 2))
    bad = rng.random(n) < outliers
    dst[bad] += rng.uniform(40.0, 200.0, (bad.sum(), 2)) * rng.choice([-1, 1], (bad.sum(), 2))
    return np.c_[src, dst].astype(np.float32), ~bad


@pytest.mark.parametrize("outliers", [0.0, 0.5])
def test_model_recovers_a_known_homography(outliers):
    rng = np.random.default_rng(3)
    H, _ = _homography(rng), None
    pts, good = _pairs(rng, H, 300, outliers)
    Hm, mask, n, best, sc = rm.ransac(pts, seed=1, max_iters=500)
    assert Hm is not None and best >= 0 and n == sc[best] == sc.max()
    assert np.array_equal(mask.astype(bool), good)
    grid = np.stack(np.meshgrid(np.linspace(-320, 320, 9), np.linspace(-240, 240, 7)), -1).reshape(-1, 2)
    assert np.abs(rm.project(Hm, grid) - rm.project(H, grid)).max() < 1e-3
    assert Hm[2, 2] == 1.0


def test_sampler_draws_distinct_indices_in_range_from_seed_and_h_alone():
    rng = np.random.default_rng(0)
    src = rng.uniform(-100, 100, (37, 2))
    pts = np.c_[src, 1.1 * src + 3.0].astype(np.float32)       # orientation-preserving
    hyps = np.arange(300)
    idx, valid = rm.draw(pts, 5, hyps)
    assert valid.all()
    assert ((idx >= 0) & (idx < 37)).all()
    assert all(len(set(r)) == 4 for r in idx.tolist())
    # h alone decides: a hypothesis drawn in another batch, or alone, is the same
    idx2, _ = rm.draw(pts, 5, hyps[::-1].copy())
    assert np.array_equal(idx2[::-1], idx)
    idx3, _ = rm.draw(pts, 5, np.array([123]))
    assert np.array_equal(idx3[0], idx[123])
    # ... and the seed changes it
    idx4, _ = rm.draw(pts, 6, hyps)
    assert not np.array_equal(idx4, idx)
    # the raw draws: 4 * 64 per hypothesis, the same in every call
    assert np.array_equal(rm.sample_indices(5, [7], 37), rm.sample_indices(5, [7], 37))


def test_sampler_is_roughly_uniform():
    count = 50
    raw = rm.sample_indices(11, np.arange(400), count).reshape(-1)[:100000]
    assert raw.size == 100000
    hist = np.bincount(raw.astype(np.int64), minlength=count)
    expect = raw.size / count
    chi2 = ((hist - expect) ** 2 / expect).sum()
    # 49 degrees of freedom: the 99.9 % quantile is 85.4
    assert chi2 < 85.4, chi2


def test_splitmix64_known_values():
    # the first outputs of splitmix64 seeded with 0 (the published reference sequence)
    state = np.array([0, rm.GAMMA, 2 * rm.GAMMA & (2 ** 64 - 1)], np.uint64)
    got = [int(v) for v in rm.splitmix64(state)]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_degeneracy_rejects_collinear_and_mirrored_quadrilaterals():
    src = np.array([[0, 0], [10, 0], [10, 10], [0, 10]], np.float64)
    idx = np.arange(4)
    assert rm.acceptable(src, src * 2 + 5, idx)
    collinear = src.copy()
    collinear[2] = [5, 0]                                       # 0, 1, 2 on one line
    assert not rm.acceptable(collinear, collinear, idx)
    assert not rm.acceptable(src, collinear, idx)
    mirrored = src * [-1, 1]
    assert not rm.acceptable(src, mirrored, idx)
    assert not rm.acceptable(src, src, np.array([0, 1, 1, 3]))   # repeated index
    nan = src.copy()
    nan[3, 0] = np.nan
    assert not rm.acceptable(src, nan, idx)


def test_solve4_is_exact_on_four_points():
    rng = np.random.default_rng(8)
    H = _homography(rng)
    src = np.array([[-200, -150], [210, -140], [190, 160], [-180, 170]], np.float64)
    dst = rm.project(H, src)
    h, ok = rm.solve4(src[None], dst[None])
    assert ok[0]
    assert np.allclose(np.r_[h[0], 1.0].reshape(3, 3), H, rtol=1e-9, atol=1e-12)
    h, ok = rm.solve4(np.zeros((1, 4, 2)), dst[None])
    assert not ok[0]


def test_too_few_or_degenerate_points_fail():
    rng = np.random.default_rng(1)
    pts = rng.uniform(-50, 50, (3, 4)).astype(np.float32)
    H, mask, n, best, sc = rm.ransac(pts, max_iters=50)
    assert H is None and n == 0 and (sc == -1).all() and not mask.any()
    line = np.zeros((40, 4), np.float32)
    line[:, 0] = line[:, 2] = np.arange(40)
    H, mask, n, best, sc = rm.ransac(line, max_iters=50)
    assert H is None and (sc == -1).all()


# ------------------------------------------------------------------ the ratio test and the packing
def test_pack_model_on_a_hand_written_example():
    kq = np.array([[0.25, 0], [1.25, -1], [2.25, -2], [3.25, -3], [4.25, -4], [5.25, -5]], np.float32)
    kt = np.array([[1000, 0.5], [1001, 1.5], [1002, 2.5], [1003, 3.5]], np.float32)
    idx = np.array([[2, 9],          # 1 < 0.5 * 4: kept
                    [0, -7],         # 2 < 0.5 * 4 is false: the comparison is strict
                    [4, 0],          # passes, but train row 4 of 4 does not exist
                    [3, 3],          # NaN
                    [1, 1],          # 3 < 0.5 * inf: kept
                    [0, 2]], np.int32)   # 1.5 < 0.5 * 3.5: kept
    dist = np.array([[1, 4], [2, 4], [0.5, 4], [np.nan, 4], [3, np.inf], [1.5, 3.5]], np.float32)
    pts, match, k = rm.pack(idx, dist, 0.5, kq, kt, 4)
    assert k == 3
    assert pts.dtype == np.float32 and match.dtype == np.int32
    assert pts.tolist() == [[0.25, 0.0, 1002.0, 2.5], [4.25, -4.0, 1001.0, 1.5],
                            [5.25, -5.0, 1000.0, 0.5]]
    assert match.tolist() == [[0, 2], [4, 1], [5, 0]]
    # one train row fewer: query 0's neighbour is out of range too
    pts, match, k = rm.pack(idx, dist, 0.5, kq, kt[:2], 2)
    assert k == 2 and match.tolist() == [[4, 1], [5, 0]]


def test_pack_model_edges():
    kq, kt = np.zeros((1, 2), np.float32), np.ones((3, 2), np.float32)

    def kept(d0, d1, t=1, ratio=0.7, nt=3):
        return rm.pack(np.array([[t, -5]], np.int32), np.array([[d0, d1]], np.float32), ratio,
                       kq, kt, nt)[2] == 1

    assert kept(0.6, 1.0) and not kept(0.8, 1.0)
    assert not kept(0.5, 1.0, ratio=0.5)                    # d0 == ratio * d1 exactly
    assert not kept(0.0, 0.0)
    assert kept(5.0, np.inf) and not kept(np.inf, np.inf)
    assert not kept(np.nan, 1.0) and not kept(0.1, np.nan) and not kept(np.nan, np.nan)
    # float32(0.7) < 0.7: in float64 this d0 is below 0.7 * 1.0, in float32 it is equal to it
    assert kept(np.float32(0.7), 1.0)
    for t in (-1, 3, 4, 2 ** 31 - 1, -2 ** 31):
        assert not kept(0.1, 1.0, t=t)
    assert kept(0.1, 1.0, t=0) and kept(0.1, 1.0, t=2)
    pts, match, k = rm.pack(np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float32), 0.7,
                            np.zeros((0, 2), np.float32), kt, 3)
    assert k == 0 and pts.shape == (0, 4) and match.shape == (0, 2)


def test_boundary_distances_sit_on_either_side_of_the_product():
    dist = rm.boundary_distances(np.random.default_rng(5), 400)
    d = dist.astype(np.float64)
    assert dist.dtype == np.float32
    assert np.all(d[0::2, 0] < 0.7 * d[0::2, 1]) and np.all(d[1::2, 0] > 0.7 * d[1::2, 1])
    up = np.nextafter(dist[0::2, 0], np.float32(np.inf)).astype(np.float64)
    down = np.nextafter(dist[1::2, 0], np.float32(-np.inf)).astype(np.float64)
    assert np.all(up >= 0.7 * d[0::2, 1]) and np.all(down <= 0.7 * d[1::2, 1])


def test_host_ratio_test_compares_in_float64():
    """``features._ratio_test`` replaces ``dist[:, 0] < ratio * dist[:, 1]`` on the float32 arrays
    of ``flann_matching``, which NumPy evaluates in float32 (ratio * d1 rounded again).  On 400
    forged boundary rows that expression drops 131 matches the contract keeps (counted below; at
    least 100 are required), so this test fails on it."""
    from pano360_amd.features import _ratio_test
    dist = rm.boundary_distances(np.random.default_rng(0), 400)
    want = np.arange(0, 400, 2)                             # the rows just below the product
    got = _ratio_test(dist, 0.7)
    assert got.dtype.kind == "i" and np.array_equal(got, want)
    _, match, k = rm.pack(np.zeros((400, 2), np.int32), dist, 0.7, np.zeros((400, 2), np.float32),
                          np.zeros((1, 2), np.float32), 1)
    assert np.array_equal(match[:, 0], got) and k == 200
    replaced = np.nonzero(dist[:, 0] < 0.7 * dist[:, 1])[0]        # the parent's expression
    differ = len(np.setxor1d(replaced, want))
    print(f"{differ} of 400 boundary rows are decided differently in float32")
    assert differ >= 100 and set(replaced) < set(want)
    assert np.array_equal(np.nonzero(rm.float32_ratio_test(dist, 0.7))[0], replaced)
    # the edges of the contract
    edge = np.array([[0.5, 1.0], [0, 0], [3, np.inf], [np.nan, 1], [1, np.nan], [0.25, 1.0],
                     [np.float32(0.7), 1.0]], np.float32)
    assert _ratio_test(edge, 0.5).tolist() == [2, 5]
    assert _ratio_test(edge, 0.7).tolist() == [0, 2, 5, 6]
    assert _ratio_test(np.zeros((0, 2), np.float32), 0.7).tolist() == []


def test_reverse():
    from pano360_amd.features import _reverse
    match = np.array([[0, 5], [3, 1], [7, 2]], np.int32)
    hom = np.array([[1.1, 0.02, 4.0], [-0.01, 0.98, -2.0], [1e-4, 2e-5, 1.0]])
    rev, inv = _reverse(match, hom)
    assert np.array_equal(rev, match[:, ::-1]) and rev.dtype == np.int32
    assert np.allclose(inv @ hom, np.eye(3))


def test_matches_npz_layout_round_trips(tmp_path):
    """What ``matching`` returns, written as features.py:320 does and read as stitcher.py:424-426
    does: 1-D keypoint array (also when every image has as many keypoints), 0-d match array whose
    item is the dict of dicts, keys in the reference's loop order."""
    from pano360_amd.features import _assemble
    rng = np.random.default_rng(4)
    n = 4
    kpts = [rng.uniform(-100, 100, (30, 2)).astype(np.float32) for _ in range(n)]
    found = {}
    for i, j in [(0, 1), (0, 3), (1, 2), (2, 3)]:              # (0, 2) and (1, 3) did not register
        mask = rng.random(30) < 0.6
        match = np.c_[np.arange(30), rng.permutation(30)].astype(np.int32)[mask]
        found[(i, j)] = (match, _homography(rng))
    kp_arr, m_arr = _assemble(kpts, found)
    assert kp_arr.shape == (n,) and kp_arr.dtype == object
    assert m_arr.shape == () and m_arr.dtype == object
    path = os.path.join(tmp_path, "matches_rig.npz")
    np.savez(path, kpts=kp_arr, matches=m_arr)
    arr = np.load(path, allow_pickle=True)
    kp2, matches = arr["kpts"], arr["matches"].item()
    assert len(kp2) == n and all(np.array_equal(a, b) and a.dtype == np.float32
                                 for a, b in zip(kp2, kpts))
    assert list(matches) == [0, 1, 3, 2]
    assert list(matches[0]) == [1, 3] and list(matches[1]) == [0, 2]
    assert list(matches[3]) == [0, 2] and list(matches[2]) == [1, 3]
    for (i, j), (match, hom) in found.items():
        m, h = matches[i][j]
        assert np.array_equal(m, match) and np.array_equal(h, hom)
        mr, hr = matches[j][i]
        assert np.array_equal(mr, match[:, ::-1]) and np.allclose(hr @ hom, np.eye(3))
        # the reference's idx_to_keypoints: query rows of image i, train rows of image j
        coords = np.concatenate([kp2[i][m[:, 0]], kp2[j][m[:, 1]]], axis=1)
        assert coords.shape == (len(m), 4)
    assert 2 not in matches[0] and 3 not in matches[1]
