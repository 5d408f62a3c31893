"""NumPy model of ``pano_match_pack`` (the ratio test and the packing, ``pack``) and of
``pano_hom_ransac`` (include/pano360.h): the sampler, the degeneracy test, the
4-point solve, the score, the selection and the refit, written from the header's contract so that
the kernel's scores can be checked bit for bit.  A test helper only: the product never imports it.

Everything the kernel evaluates in float32 is evaluated here on float32 arrays, one operation at
a time in the header's order (the library builds with -ffp-contract=off); the f64 solve repeats
the kernel's operation order.  The refit is the same Hartley-normalised DLT, solved with
``np.linalg.eigh``: the same matrix up to the order of its sums, so it agrees to rounding only."""
import numpy as np

GAMMA = 0x9E3779B97F4A7C15
MAX_ATTEMPTS = 64
TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))
_U64 = np.uint64


def pack(idx, dist, ratio, kp_query, kp_train, nt):
    """``pano_match_pack`` (include/pano360.h) for one pair: query q survives iff
    float64(dist[q, 0]) < ratio * float64(dist[q, 1]) - strict, so a NaN on either side drops
    it - and 0 <= idx[q, 0] < nt; the survivors come in ascending q.  idx int32 [nq][2] and
    dist float32 [nq][2] as pano_knn2 leaves them, kp_query float32 [nq][2], kp_train float32
    [nt][2].  Returns (pts float32 [k][4]: the query keypoint, then its nearest train keypoint;
    match int32 [k][2]: q, idx[q, 0]; k)."""
    idx = np.asarray(idx, np.int32).reshape(-1, 2)
    dist = np.asarray(dist, np.float32).reshape(-1, 2).astype(np.float64)
    kq = np.asarray(kp_query, np.float32).reshape(-1, 2)
    kt = np.asarray(kp_train, np.float32).reshape(-1, 2)
    t = idx[:, 0].astype(np.int64)
    with np.errstate(invalid="ignore"):
        keep = (dist[:, 0] < np.float64(ratio) * dist[:, 1]) & (t >= 0) & (t < nt)
    q = np.nonzero(keep)[0]
    pts = np.concatenate([kq[q], kt[t[q]]], axis=1).astype(np.float32).reshape(-1, 4)
    match = np.stack([q, t[q]], axis=1).astype(np.int32).reshape(-1, 2)
    return pts, match, len(q)


def boundary_distances(rng, n, ratio=0.7):
    """Forged (d0, d1) float32 [n][2] on the boundary of the ratio test: d1 random in [0.1, 2),
    d0 the float32 just below (even rows) or just above (odd rows) the float64 product
    ratio * d1.  In float64 the even rows pass and the odd rows fail; a comparison in float32
    rounds ratio * d1 once more and decides many of them the other way."""
    d1 = rng.uniform(0.1, 2.0, n).astype(np.float32)
    prod = np.float64(ratio) * d1.astype(np.float64)
    near = prod.astype(np.float32)
    below = np.where(near.astype(np.float64) < prod, near, np.nextafter(near, np.float32(-np.inf)))
    above = np.where(near.astype(np.float64) > prod, near, np.nextafter(near, np.float32(np.inf)))
    d0 = np.where(np.arange(n) % 2 == 0, below, above).astype(np.float32)
    return np.stack([d0, d1], axis=1)


def float32_ratio_test(dist, ratio):
    """The comparison as NumPy evaluates it on float32 arrays (ratio * d1 rounded to float32):
    NOT the contract; the tests count the rows on which it differs from the contract."""
    dist = np.asarray(dist, np.float32)
    with np.errstate(invalid="ignore"):
        return dist[:, 0] < np.float32(ratio) * dist[:, 1]


def splitmix64(x):
    """splitmix64's output for the state ``x`` (uint64 array): the state advanced by the golden
    gamma, then the two xor-shift-multiply rounds."""
    with np.errstate(over="ignore"):
        z = np.asarray(x, np.uint64) + _U64(GAMMA)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        return z ^ (z >> _U64(31))


def sample_indices(seed, hyps, count, attempts=MAX_ATTEMPTS):
    """[len(hyps)][attempts][4] candidate indices in [0, count): draw k of attempt a of
    hypothesis h is ((r >> 32) * count) >> 32 with
    r = splitmix64(seed + GAMMA * (h * 256 + a * 4 + k + 1))."""
    h = np.asarray(hyps, np.uint64)[:, None, None]
    a = np.arange(attempts, dtype=np.uint64)[None, :, None]
    k = np.arange(4, dtype=np.uint64)[None, None, :]
    with np.errstate(over="ignore"):
        key = _U64(seed & 0xFFFFFFFFFFFFFFFF) + _U64(GAMMA) * (h * _U64(256) + a * _U64(4) + k + _U64(1))
    r = splitmix64(key)
    return ((r >> _U64(32)) * _U64(count)) >> _U64(32)


def signed_area(p, a, b, c):
    """Twice the signed area of the triangle p[a] p[b] p[c] (f64, this operation order)."""
    return ((p[..., b, 0] - p[..., a, 0]) * (p[..., c, 1] - p[..., a, 1])
            - (p[..., b, 1] - p[..., a, 1]) * (p[..., c, 0] - p[..., a, 0]))


def acceptable(src, dst, idx):
    """The degeneracy test of a draw: four distinct indices and, for every triple, src and dst
    triangles of the same strict orientation (the product of their signed areas > 0; a NaN
    rejects).  src, dst: f64 [..., 4, 2] of the drawn points."""
    i = idx
    distinct = ((i[..., 0] != i[..., 1]) & (i[..., 0] != i[..., 2]) & (i[..., 0] != i[..., 3])
                & (i[..., 1] != i[..., 2]) & (i[..., 1] != i[..., 3]) & (i[..., 2] != i[..., 3]))
    ok = distinct
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b, c in TRIPLES:
            ok = ok & (signed_area(src, a, b, c) * signed_area(dst, a, b, c) > 0)
    return ok


def draw(pts, seed, hyps):
    """(sample indices [H][4] int64, valid [H]) of hypotheses ``hyps`` of one pair (pts float32
    [m][4]): the first acceptable attempt of each, invalid after MAX_ATTEMPTS."""
    m = len(pts)
    idx = sample_indices(seed, hyps, m).astype(np.int64)          # [H][A][4]
    p = pts.astype(np.float64)[idx]                               # [H][A][4][4]
    ok = acceptable(p[..., 0:2], p[..., 2:4], idx)
    first = np.argmax(ok, axis=1)
    valid = ok[np.arange(len(hyps)), first]
    return idx[np.arange(len(hyps)), first], valid


def solve4(src, dst):
    """Exact homography (h33 = 1) of four correspondences, f64 [H][4][2] each: the 8 x 8 system,
    Gaussian elimination with partial pivoting (the first maximal |pivot|), back substitution.
    Returns (h [H][8] f64, valid [H]): a zero or non-finite pivot invalidates."""
    n = src.shape[0]
    A = np.zeros((n, 8, 9))
    x, y, u, v = src[..., 0], src[..., 1], dst[..., 0], dst[..., 1]
    for i in range(4):
        r0, r1 = 2 * i, 2 * i + 1
        A[:, r0, 0], A[:, r0, 1], A[:, r0, 2] = x[:, i], y[:, i], 1.0
        A[:, r0, 6], A[:, r0, 7], A[:, r0, 8] = -(u[:, i] * x[:, i]), -(u[:, i] * y[:, i]), u[:, i]
        A[:, r1, 3], A[:, r1, 4], A[:, r1, 5] = x[:, i], y[:, i], 1.0
        A[:, r1, 6], A[:, r1, 7], A[:, r1, 8] = -(v[:, i] * x[:, i]), -(v[:, i] * y[:, i]), v[:, i]
    valid = np.ones(n, bool)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        for c in range(8):
            p = c + np.argmax(np.abs(A[:, c:, c]), axis=1)
            piv = A[rows, p, c]
            valid &= np.isfinite(piv) & (np.abs(piv) > 0)
            top = A[rows, c, :].copy()
            A[rows, c, :] = A[rows, p, :]
            A[rows, p, :] = top
            for r in range(c + 1, 8):
                f = A[:, r, c] / A[:, c, c]
                A[:, r, c + 1:] = A[:, r, c + 1:] - f[:, None] * A[:, c, c + 1:]
        h = np.zeros((n, 8))
        for r in range(7, -1, -1):
            s = A[:, r, 8].copy()
            for k in range(r + 1, 8):
                s = s - A[:, r, k] * h[:, k]
            h[:, r] = s / A[:, r, r]
    return h, valid


def inliers(hf, pts, t2):
    """The float32 test of hypotheses hf (float32 [H][8], h33 = 1) on pts float32 [m][4]:
    bool [H][m]."""
    f32 = np.float32
    x, y, u, v = (pts[None, :, k] for k in range(4))
    H = [hf[:, k:k + 1] for k in range(8)]
    with np.errstate(all="ignore"):
        ww = f32(1) / ((H[6] * x + H[7] * y) + f32(1))
        dx = ((H[0] * x + H[1] * y) + H[2]) * ww - u
        dy = ((H[3] * x + H[4] * y) + H[5]) * ww - v
        err = dx * dx + dy * dy
        return err <= t2


def thresh2(thresh):
    return np.float32(np.float64(np.float32(thresh)) ** 2)


def hypotheses(pts, seed, max_iters):
    """(h f64 [H][8], valid [H], sample [H][4]) of every hypothesis of one pair."""
    hyps = np.arange(max_iters)
    idx, valid = draw(pts, seed, hyps)
    p = pts.astype(np.float64)[idx]
    h, ok = solve4(p[..., 0:2], p[..., 2:4])
    return h, valid & ok, idx


def scores(pts, seed, max_iters, thresh):
    """Inlier count of every hypothesis (-1: invalid), as the kernel's ``hyp_inliers``."""
    pts = np.ascontiguousarray(pts, np.float32)
    if len(pts) < 4:
        return np.full(max_iters, -1, np.int32)
    h, valid, _ = hypotheses(pts, seed, max_iters)
    with np.errstate(all="ignore"):
        hf = h.astype(np.float32)
    t2 = thresh2(thresh)
    out = np.empty(max_iters, np.int32)
    for s in range(0, max_iters, 128):
        out[s:s + 128] = inliers(hf[s:s + 128], pts, t2).sum(axis=1)
    out[~valid] = -1
    return out


def normalise(p):
    """Hartley: centroid to the origin, mean distance sqrt(2).  (scale, cx, cy)."""
    c = p.mean(axis=0)
    d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    return np.sqrt(2.0) / d, c[0], c[1]


def refit(src, dst):
    """Hartley-normalised DLT over the inliers (f64 [n][2] each): the eigenvector of the smallest
    eigenvalue of the 9 x 9 normal matrix, denormalised, h33 = 1."""
    s1, cx, cy = normalise(src)
    s2, cu, cv = normalise(dst)
    x, y = (src[:, 0] - cx) * s1, (src[:, 1] - cy) * s1
    u, v = (dst[:, 0] - cu) * s2, (dst[:, 1] - cv) * s2
    z, o = np.zeros_like(x), np.ones_like(x)
    a1 = np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], axis=1)
    a2 = np.stack([z, z, z, x, y, o, -v * x, -v * y, -v], axis=1)
    M = a1.T @ a1 + a2.T @ a2
    _, vec = np.linalg.eigh(M)
    hn = vec[:, 0].reshape(3, 3)
    t1 = np.array([[s1, 0, -s1 * cx], [0, s1, -s1 * cy], [0, 0, 1]])
    t2inv = np.array([[1 / s2, 0, cu], [0, 1 / s2, cv], [0, 0, 1]])
    H = t2inv @ hn @ t1
    return H / H[2, 2]


def ransac(pts, seed=0, max_iters=2000, thresh=3.0):
    """The whole contract for one pair: (H (3, 3) f64 or None, mask uint8 [m], n_inliers,
    best hypothesis index or -1, scores [max_iters])."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    sc = scores(pts, seed, max_iters, thresh)
    m = len(pts)
    best = int(np.argmax(sc))            # the first maximum: the lowest h of a tie
    if m < 4 or sc[best] < 4:
        return None, np.zeros(m, np.uint8), 0, -1, sc
    h, _, _ = hypotheses(pts, seed, best + 1)
    with np.errstate(all="ignore"):
        hf = h[best:best + 1].astype(np.float32)
    mask = inliers(hf, pts, thresh2(thresh))[0]
    p = pts.astype(np.float64)
    H = refit(p[mask, 0:2], p[mask, 2:4])
    if not np.all(np.isfinite(H)):
        return None, np.zeros(m, np.uint8), 0, best, sc
    return H, mask.astype(np.uint8), int(sc[best]), best, sc


def project(H, p):
    """Apply H (3, 3) to points [n][2] (f64)."""
    q = np.c_[p, np.ones(len(p))] @ np.asarray(H, np.float64).T
    return q[:, :2] / q[:, 2:3]
