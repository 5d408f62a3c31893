"""A NumPy statement of ``pano_photo_stats`` and ``pano_photo_apply_u8`` (include/pano360.h) and
of the fit around them, written from the contract and independent of pano360_amd/photo.py: every
float64 operation rounded once, in the order written there; the sampling in float32.

The device and NumPy evaluate the same operations; only ``log`` may differ, by a few units in the
last place.  No decision depends on it: positions, taps and the range test use exactly rounded
operations only (+, -, *, /, rint), so both sides count the same samples.  ``stats`` also returns,
for every sum, the sum of the absolute values of its terms: the scale a comparison of two
summation orders is measured in."""
import numpy as np

SUMS = 25
TABLE = 1026
EE = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # sums 4 .. 9


def homography(rot_i, intr_i, rot_j, intr_j):
    """Centred pixels of frame i -> centred pixels of frame j: (K_j R_j)(R_i^T K_i^-1)."""
    return (np.asarray(intr_j, np.float64) @ np.asarray(rot_j, np.float64)) @ \
        (np.asarray(rot_i, np.float64).T @ np.linalg.inv(np.asarray(intr_i, np.float64)))


def all_pairs(rots, intrs):
    """Every (i, j, H) with i < j: the model takes no shortcut."""
    n = len(rots)
    return [(i, j, homography(rots[i], intrs[i], rots[j], intrs[j]))
            for i in range(n) for j in range(i + 1, n)]


def rho_of(a, b, w, h):
    """rho of positions whose doubled, centred coordinates are (a, b) = (2x + 1 - w, 2y + 1 - h)."""
    return (a * a + b * b) / np.float64(w * w + h * h)


def rho_grid(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return rho_of((2 * x + 1 - w).astype(np.float64), (2 * y + 1 - h).astype(np.float64), w, h)


def samples(frame_i, frame_j, H, lo, hi, step):
    """The samples of one pair that count: (x, y, v_i float64 [m][3], v_j float64 [m][3], rho_i,
    rho_j)."""
    hi_, wi = frame_i.shape[:2]
    hj, wj = frame_j.shape[:2]
    H = np.asarray(H, np.float64).ravel()
    y, x = np.mgrid[0:hi_:step, 0:wi:step]
    x, y = x.ravel(), y.ravel()
    xc = x.astype(np.float64) - np.float64(wi) / 2.0
    yc = y.astype(np.float64) - np.float64(hi_) / 2.0
    X = (H[0] * xc + H[1] * yc) + H[2]
    Y = (H[3] * xc + H[4] * yc) + H[5]
    Z = (H[6] * xc + H[7] * yc) + H[8]
    keep = Z > 0
    x, y, X, Y, Z = x[keep], y[keep], X[keep], Y[keep], Z[keep]
    with np.errstate(over="ignore", invalid="ignore"):
        px = X / Z + np.float64(wj) / 2.0
        py = Y / Z + np.float64(hj) / 2.0
        keep = (px >= 0) & (px <= wj - 1) & (py >= 0) & (py <= hj - 1)
    x, y, px, py = x[keep], y[keep], px[keep], py[keep]
    sx = np.rint(32.0 * px).astype(np.int64)
    sy = np.rint(32.0 * py).astype(np.int64)
    ix = np.minimum(sx >> 5, wj - 2)
    iy = np.minimum(sy >> 5, hj - 2)
    tx = ((sx - 32 * ix).astype(np.float32) / np.float32(32))[:, None]
    ty = ((sy - 32 * iy).astype(np.float32) / np.float32(32))[:, None]
    one = np.float32(1)
    fj = frame_j.astype(np.float32)
    top = fj[iy, ix] * (one - tx) + fj[iy, ix + 1] * tx
    bot = fj[iy + 1, ix] * (one - tx) + fj[iy + 1, ix + 1] * tx
    vj = top * (one - ty) + bot * ty
    assert vj.dtype == np.float32
    vi = frame_i[y, x].astype(np.float32)
    keep = ((vi >= lo) & (vi <= hi) & (vj >= lo) & (vj <= hi)).all(axis=1)
    x, y, sx, sy, vi, vj = x[keep], y[keep], sx[keep], sy[keep], vi[keep], vj[keep]
    rho_i = rho_of((2 * x + 1 - wi).astype(np.float64), (2 * y + 1 - hi_).astype(np.float64), wi, hi_)
    qx, qy = sx.astype(np.float64) / 32.0, sy.astype(np.float64) / 32.0
    rho_j = rho_of((2.0 * qx + 1.0) - np.float64(wj), (2.0 * qy + 1.0) - np.float64(hj), wj, hj)
    return x, y, vi.astype(np.float64), vj.astype(np.float64), rho_i, rho_j


def pair_sums(frame_i, frame_j, H, lo, hi, step, dlg=(0.0, 0.0, 0.0), alpha=(0.0, 0.0, 0.0),
              tau=np.inf):
    """(the 25 sums, the 25 sums of the terms' absolute values) of one pair."""
    _, _, vi, vj, rho_i, rho_j = samples(frame_i, frame_j, H, lo, hi, step)
    a1, a2, a3 = (np.float64(a) for a in alpha)
    d = np.log(vi) - np.log(vj)
    e = np.stack([rho_i - rho_j, rho_i * rho_i - rho_j * rho_j,
                  (rho_i * rho_i) * rho_i - (rho_j * rho_j) * rho_j], axis=1)
    fall = (a1 * e[:, 0] + a2 * e[:, 1]) + a3 * e[:, 2]
    res = (d - np.asarray(dlg, np.float64)[None, :]) - fall[:, None]
    m = np.abs(res).max(axis=1) if len(res) else np.zeros(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        wt = np.where(m > tau, np.float64(tau) / m, 1.0)
    terms = [wt]
    we = wt[:, None] * e
    terms += [we[:, k] for k in range(3)]
    terms += [we[:, k] * e[:, m_] for k, m_ in EE]
    for c in range(3):
        wd = wt * d[:, c]
        terms += [wd, wd * e[:, 0], wd * e[:, 1], wd * e[:, 2], wd * d[:, c]]
    terms = np.stack(terms, axis=1) if len(wt) else np.zeros((0, SUMS))
    assert terms.shape[1] == SUMS
    return terms.sum(axis=0), np.abs(terms).sum(axis=0)


def stats(frames, pairs, lo, hi, step, log_gains=None, alpha=(0.0, 0.0, 0.0), tau=np.inf):
    """(sums float64 [P][25], their absolute scales [P][25]) of the pairs (i, j, H)."""
    lg = np.zeros((len(frames), 3)) if log_gains is None else np.asarray(log_gains, np.float64)
    out = [pair_sums(frames[i], frames[j], H, lo, hi, step, lg[i] - lg[j], alpha, tau)
           for i, j, H in pairs]
    if not out:
        return np.zeros((0, SUMS)), np.zeros((0, SUMS))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def solve(n, pairs, sums, terms, prior=1e-4):
    """(log_gains [n][3], alpha [3]): the normal equations assembled from design rows - a
    sample of pair (i, j) in channel c has +1 at (i, c), -1 at (j, c) and e_k at alpha_k -, the
    ridge prior * sum(w) / n on the log-gains, each channel's mean subtracted afterwards."""
    size = 3 * n + terms
    A, b = np.zeros((size, size)), np.zeros(size)
    total = sum(S[0] for S in sums)
    if not total > 0:
        return np.zeros((n, 3)), np.zeros(3)
    for (i, j, _), S in zip(pairs, sums):
        see = np.zeros((3, 3))
        for idx, (k, m) in enumerate(EE):
            see[k, m] = see[m, k] = S[4 + idx]
        for c in range(3):
            # second moments of the design row (u = +1, v = -1, e_1 .. e_terms) and its product with d
            cols = [3 * i + c, 3 * j + c] + [3 * n + k for k in range(terms)]
            mom = np.zeros((2 + terms, 2 + terms))
            mom[0, 0] = mom[1, 1] = S[0]
            mom[0, 1] = mom[1, 0] = -S[0]
            for k in range(terms):
                mom[0, 2 + k] = mom[2 + k, 0] = S[1 + k]
                mom[1, 2 + k] = mom[2 + k, 1] = -S[1 + k]
                for m in range(terms):
                    mom[2 + k, 2 + m] = see[k, m]
            rhs = np.array([S[10 + 5 * c], -S[10 + 5 * c]] + [S[11 + 5 * c + k] for k in range(terms)])
            A[np.ix_(cols, cols)] += mom
            b[cols] += rhs
    A[np.arange(3 * n), np.arange(3 * n)] += prior * total / n
    theta = np.linalg.solve(A, b)
    lg = theta[:3 * n].reshape(n, 3)
    alpha = np.zeros(3)
    alpha[:terms] = theta[3 * n:]
    return lg - lg.mean(axis=0, keepdims=True), alpha


def estimate(frames, pairs, terms, rounds=2, tau=0.05, lo=16, hi=239, step=1, prior=1e-4):
    """The passes: every weight 1, then ``rounds`` reweighted ones.  Returns (log_gains, alpha,
    the first pass's (log_gains, alpha))."""
    sums, _ = stats(frames, pairs, lo, hi, step)
    lg, alpha = solve(len(frames), pairs, sums, terms, prior)
    first = (lg, alpha)
    for _ in range(rounds):
        sums, _ = stats(frames, pairs, lo, hi, step, lg, alpha, tau)
        lg, alpha = solve(len(frames), pairs, sums, terms, prior)
    return lg, alpha, first


def log_falloff(alpha, rho):
    a1, a2, a3 = (np.float64(a) for a in alpha)
    rho = np.asarray(rho, np.float64)
    return (a1 * rho + a2 * (rho * rho)) + a3 * ((rho * rho) * rho)


def table(log_gain, alpha):
    """float32 [3][1026] of one camera: T[c][k] = float32(exp(-lg[c] - log V(k / 1024)))."""
    rho = np.arange(TABLE, dtype=np.float64) / 1024.0
    fall = log_falloff(alpha, rho)
    return np.exp(-np.asarray(log_gain, np.float64)[:, None] - fall[None, :]).astype(np.float32)


def apply(frame, T):
    """The corrected uint8 frame: per pixel the factor from ``T``, linear in 1024 rho, in float32
    without a fused multiply-add; rint(min(v f, 255))."""
    h, w = frame.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    dx, dy = (2 * x + 1 - w).astype(np.int64), (2 * y + 1 - h).astype(np.int64)
    s = (dx * dx + dy * dy).astype(np.float64) / np.float64(w * w + h * h) * 1024.0
    k = s.astype(np.int64)
    t = (s - k.astype(np.float64)).astype(np.float32)
    out = np.empty_like(frame)
    for c in range(3):
        f0, f1 = T[c][k], T[c][k + 1]
        f = f0 + t * (f1 - f0)
        value = frame[..., c].astype(np.float32) * f
        assert value.dtype == np.float32
        out[..., c] = np.rint(np.minimum(value, np.float32(255))).astype(np.uint8)
    return out


def overlap_difference(frames, pairs, step=1):
    """The mean absolute difference, in levels, between frame i's bytes and frame j's bilinear
    samples over every sample of every pair (no range test: lo = 0, hi = 255)."""
    total, count = 0.0, 0
    for i, j, H in pairs:
        _, _, vi, vj, _, _ = samples(frames[i], frames[j], H, 0, 255, step)
        total += np.abs(vi - vj).sum()
        count += vi.size
    return total / max(count, 1)
