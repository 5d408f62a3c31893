"""NumPy restatement of the refinement contract (include/pano360.h, pano_ba_refine) and of the
Levenberg-Marquardt loop of ``bundle_adj.refine``, independent of the product: the residual under
the shared radial distortion, its analytic Jacobian by the chain rule in matrix form, the Huber
weights, the per-pair sums together with the sums of their terms' absolute values, the loop, and
the forward distortion that forges data.  Test helper only: the product never imports it."""
import numpy as np

NEWTON = 10
TERMS = 70


def rodrigues(w):
    w = np.asarray(w, np.float64)
    ang = np.linalg.norm(w)
    if ang == 0:
        return np.eye(3)
    a = w / ang
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def forward(p, k):
    """Undistorted normalised points [.., 2] -> distorted ones: p (1 + k1 r^2 + k2 r^4)."""
    p = np.asarray(p, np.float64)
    r2 = np.sum(p * p, axis=-1, keepdims=True)
    return p * (1 + k[0] * r2 + k[1] * r2 * r2)


def distort_pixels(xy, focal, k):
    """Centred pixels of an ideal camera of focal length ``focal`` -> the distorted one's."""
    return forward(np.asarray(xy, np.float64) / focal, k) * focal


def undist(cam, xy, k):
    """cam = (f, px, py); xy [M][2] centred pixels.  Returns d, u [M][2], r, rd, h' at the solution
    [M], and whether every h' met was positive."""
    f, px, py = cam
    with np.errstate(all="ignore"):
        d = (np.asarray(xy, np.float64) - [px, py]) / f
        rd = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        r = rd.copy()
        ok = np.ones(len(d), bool)
        for _ in range(NEWTON):
            q = r * r
            q2 = q * q
            h = r * ((1 + k[0] * q) + k[1] * q2)
            hp = (1 + (3 * k[0]) * q) + (5 * k[1]) * q2
            ok &= hp > 0
            r = r - (h - rd) / hp
        q = r * r
        hp = (1 + (3 * k[0]) * q) + (5 * k[1]) * (q * q)
        ok &= hp > 0
        s = np.where(rd > 0, r / np.where(rd > 0, rd, 1), 1.0)
    return d, s[:, None] * d, r, rd, hp, ok


def rotate(Ra, Rb, w):
    """R_b (R_a^T w) for w [M][3] in the contract's order, (m0 w0 + m1 w1) + m2 w2 per row,
    elementwise: no matrix product, whose rounding depends on the BLAS at hand."""
    t = [(Ra[0, r] * w[:, 0] + Ra[1, r] * w[:, 1]) + Ra[2, r] * w[:, 2] for r in range(3)]
    return np.stack([(Rb[r, 0] * t[0] + Rb[r, 1] * t[1]) + Rb[r, 2] * t[2] for r in range(3)],
                    axis=1)


def residual(cam_a, Ra, cam_b, Rb, rows, k):
    """e [M][2] and the validity that does not depend on J: rows [M][4] = (x_b, y_b, x_a, y_a)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        _, ub, _, _, _, okb = undist(cam_b, rows[:, 0:2], k)
        _, ua, _, _, _, oka = undist(cam_a, rows[:, 2:4], k)
        q = np.c_[ua, np.ones(len(ua))]
        v = rotate(Ra, Rb, q)
        pi = v[:, :2] * (1.0 / v[:, 2:])
        e = cam_b[0] * (ub - pi)
    return e, okb & oka & (v[:, 2] > 0)


def _du(cam, d, r, rd, hp, k):
    """Per match: du/dd [M][2][2], du/df [M][2], du/dk [M][2][2] (last axis k1, k2), by the
    implicit function theorem on r (1 + k1 r^2 + k2 r^4) = rd."""
    M = len(d)
    pos = rd > 0
    safe = np.where(pos, rd, 1.0)
    s = np.where(pos, r / safe, 1.0)
    # u = (r(rd) / rd) d: du/dd = s I + (r' rd - r) / rd^3 d d^T, r' = 1 / h'
    coef = np.where(pos, (safe / hp - r) / safe ** 3, 0.0)
    du_dd = s[:, None, None] * np.eye(2) + coef[:, None, None] * d[:, :, None] * d[:, None, :]
    du_df = np.einsum("mij,mj->mi", du_dd, -d / cam[0])
    unit = np.where(pos[:, None], d / safe[:, None], 0.0)
    du_dk = np.stack([unit * (-(r ** 3) / hp)[:, None], unit * (-(r ** 5) / hp)[:, None]], axis=2)
    assert du_dk.shape == (M, 2, 2)
    return du_dd, du_df, du_dk


def jacobian(cam_a, Ra, cam_b, Rb, rows, k):
    """J [M][2][10] by (f_b, omega_b, f_a, omega_a, k1, k2), e [M][2], valid [M]."""
    rows = np.asarray(rows, np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        db, ub, rb, rdb, hpb, okb = undist(cam_b, rows[:, 0:2], k)
        da, ua, ra, rda, hpa, oka = undist(cam_a, rows[:, 2:4], k)
        _, dub_df, dub_dk = _du(cam_b, db, rb, rdb, hpb, k)
        _, dua_df, dua_dk = _du(cam_a, da, ra, rda, hpa, k)
        fb = cam_b[0]
        Mab = Rb @ Ra.T
        q = np.c_[ua, np.ones(len(ua))]
        v = rotate(Ra, Rb, q)
        pi = v[:, :2] * (1.0 / v[:, 2:])
        e = fb * (ub - pi)
        # d pi / d v [M][2][3]
        P = np.zeros((len(v), 2, 3))
        P[:, 0, 0] = P[:, 1, 1] = 1 / v[:, 2]
        P[:, 0, 2], P[:, 1, 2] = -v[:, 0] / v[:, 2] ** 2, -v[:, 1] / v[:, 2] ** 2
        eye = np.eye(3)
        J = np.zeros((len(v), 2, 10))
        J[:, :, 0] = (ub - pi) + fb * dub_df
        for t in range(3):
            dv = np.cross(eye[t], v)                         # exp([w]x) R_b: v + w x v
            J[:, :, 1 + t] = -fb * np.einsum("mij,mj->mi", P, dv)
            dv = -np.cross(eye[t], q) @ Mab.T                # R_a^T exp(-[w]x): M (q - w x q)
            J[:, :, 5 + t] = -fb * np.einsum("mij,mj->mi", P, dv)
        dq = np.c_[dua_df, np.zeros(len(v))]
        J[:, :, 4] = -fb * np.einsum("mij,mj->mi", P, dq @ Mab.T)
        for t in range(2):
            dq = np.c_[dua_dk[:, :, t], np.zeros(len(v))]
            J[:, :, 8 + t] = fb * (dub_dk[:, :, t] - np.einsum("mij,mj->mi", P, dq @ Mab.T))
        valid = okb & oka & (v[:, 2] > 0)
        valid &= np.all(np.isfinite(e), axis=1) & np.all(np.isfinite(J), axis=(1, 2))
    return J, e, valid


def huber(e, delta):
    """(w, rho, n) per match."""
    n = np.sqrt(np.sum(e * e, axis=1))
    inl = n <= delta
    safe = np.where(inl, 1.0, n)
    return np.where(inl, 1.0, delta / safe), np.where(inl, n * n / 2, delta * (n - delta / 2)), n


def pair_sums(rows, pairs, cams, k, delta):
    """out [P][70] as include/pano360.h lays it out, and per entry the sum of the absolute values
    of the per-match terms that are summed into it (the counts' are the counts)."""
    rows = np.asarray(rows, np.float64)
    cams = np.asarray(cams, np.float64).reshape(-1, 12)
    iu, iv = np.triu_indices(10)
    out, mag = np.zeros((len(pairs), TERMS)), np.zeros((len(pairs), TERMS))
    for p, (a, b, first, count) in enumerate(np.asarray(pairs).tolist()):
        m = rows[first:first + count]
        J, e, valid = jacobian(cams[a, :3], cams[a, 3:].reshape(3, 3), cams[b, :3],
                               cams[b, 3:].reshape(3, 3), m, k)
        out[p, 67] = mag[p, 67] = np.sum(~valid)
        J, e = J[valid], e[valid]
        w, rho, n = huber(e, delta)
        jtj = np.einsum("m,mic,mie->mce", w, J, J)[:, iu, iv]
        jte = np.einsum("m,mic,mi->mc", w, J, e)
        inl = n <= delta
        rest = np.stack([rho, w, np.zeros(len(w)), np.where(inl, n * n, 0.0), inl * 1.0], axis=1)
        terms = np.concatenate([jtj, jte, rest], axis=1)
        keep = np.arange(TERMS) != 67
        out[p, keep] = np.sum(terms, axis=0)[keep]
        mag[p, keep] = np.sum(np.abs(terms), axis=0)[keep]
    return out, mag


# ------------------------------------------------------------------ the loop
def pairs_of(matches, index):
    """[(a, b, rows [M][4])] of bundle_adj.refine: every unordered pair once, ascending (i, j),
    b = i's camera, a = j's."""
    slot = {int(img): c for c, img in enumerate(index)}
    out = []
    for i in sorted(matches):
        for j in sorted(matches[i]):
            if i < j and i in slot and j in slot:
                m = np.asarray(matches[i][j][0], np.float64)
                out.append((slot[j], slot[i], m[:, [0, 1, 3, 4]]))
    return out


def table_of(pairs):
    """(rows [m][4], pair table int32 [P][4]) of a list of (a, b, rows)."""
    first = np.cumsum([0] + [len(r) for _, _, r in pairs])
    table = np.array([(a, b, first[p], len(r)) for p, (a, b, r) in enumerate(pairs)], np.int32)
    return np.concatenate([r for _, _, r in pairs]), table.reshape(-1, 4)


def reduction(n, table, lens_terms, shared_focal):
    """T [4 n + 2][size] of 0 / 1: full parameters (camera c: f, omega at 4 c ..; k last) from the
    reduced ones.  The rotation of the first camera with a match, cameras without a match and the
    k not estimated have no column; with shared_focal every f shares column 0."""
    used = np.zeros(n, bool)
    for a, b, _, count in table.tolist():
        if count:
            used[a] = used[b] = True
    cols = []
    gauge = min(c for c in range(n) if used[c])
    if shared_focal:
        cols.append([4 * c for c in range(n) if used[c]])
    for c in range(n):
        if not used[c]:
            continue
        if not shared_focal:
            cols.append([4 * c])
        if c != gauge:
            cols += [[4 * c + 1], [4 * c + 2], [4 * c + 3]]
    cols += [[4 * n + t] for t in range(lens_terms)]
    T = np.zeros((4 * n + 2, len(cols)))
    for j, members in enumerate(cols):
        T[members, j] = 1
    return T


def full_system(out, table, n):
    """The (4 n + 2)^2 system of the per-pair blocks, the pairs added in order."""
    size = 4 * n + 2
    A, g = np.zeros((size, size)), np.zeros(size)
    iu, iv = np.triu_indices(10)
    for p, (a, b, _, _) in enumerate(table.tolist()):
        where = np.array([4 * b, 4 * b + 1, 4 * b + 2, 4 * b + 3, 4 * a, 4 * a + 1, 4 * a + 2,
                          4 * a + 3, 4 * n, 4 * n + 1])
        blk = np.zeros((10, 10))
        blk[iu, iv] = out[p, :55]
        blk = blk + np.triu(blk, 1).T
        A[np.ix_(where, where)] += blk
        g[where] += out[p, 55:65]
    return A, g


def totals(out):
    return (float(np.sum(out[:, 65])), int(round(np.sum(out[:, 67]))), float(np.sum(out[:, 68])),
            int(round(np.sum(out[:, 69]))))


def lm(f, pp, R, rows, table, *, lens_terms=0, shared_focal=None, delta=3.0, max_iter=100,
       sums=None):
    """The loop of bundle_adj.refine on ``sums(cams [n][12], k) -> out`` (default: this model's
    pair_sums).  Returns a dict: f, R, k, history [(cost, lambda, accepted)], rms_before,
    rms_after, inlier_share, n_invalid."""
    n = len(f)
    if shared_focal is None:
        shared_focal = lens_terms > 0
    if sums is None:
        def sums(cams, k):
            return pair_sums(rows, table, cams, k, delta)[0]
    f, R, k = np.array(f, np.float64), np.array(R, np.float64), np.zeros(2)
    if shared_focal:
        f[:] = np.median(f)
    pp = np.asarray(pp, np.float64)

    def state(f, R):
        return np.concatenate([f[:, None], pp, R.reshape(n, 9)], axis=1)

    T = reduction(n, table, lens_terms, shared_focal)
    cur = sums(state(f, R), k)
    cost, invalid, ssq, inl = totals(cur)
    rms_before = np.sqrt(ssq / inl) if inl else np.nan
    history, lam = [], 1e-3
    for _ in range(max_iter):
        if lam > 1e12:
            break
        A, g = full_system(cur, table, n)
        A, g = T.T @ A @ T, T.T @ g
        try:
            step = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
        except np.linalg.LinAlgError:
            step = np.full(len(g), np.nan)
        if not np.all(np.isfinite(step)):
            history.append((np.nan, lam, False))
            lam *= 10
            continue
        full = T @ step
        f_c = f + full[0:4 * n:4]
        R_c = np.stack([rodrigues(full[4 * c + 1:4 * c + 4]) @ R[c] for c in range(n)])
        k_c = k + full[4 * n:]
        cand = sums(state(f_c, R_c), k_c)
        c_cost, c_invalid, c_ssq, c_inl = totals(cand)
        keep = bool(c_cost < cost and c_invalid <= invalid)
        history.append((c_cost, lam, keep))
        if keep:
            decrease = (cost - c_cost) / cost
            f, R, k, cur = f_c, R_c, k_c, cand
            cost, invalid, ssq, inl = c_cost, c_invalid, c_ssq, c_inl
            lam /= 10
            if decrease < 1e-10:
                break
        else:
            lam *= 10
    return {"f": f, "R": R, "k": k, "history": history, "rms_before": float(rms_before),
            "rms_after": float(np.sqrt(ssq / inl)) if inl else float("nan"),
            "inlier_share": inl / int(np.sum(table[:, 3])), "n_invalid": invalid}


def rotation_distance(R, R_true):
    """The largest angle (radians) between R[c] and R_true[c] G, G the common rotation that takes
    camera 0's truth to its estimate."""
    G = R_true[0].T @ R[0]
    worst = 0.0
    for est, true in zip(R, R_true):
        d = est @ (true @ G).T
        axis = 0.5 * np.array([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]])
        worst = max(worst, float(np.arctan2(np.linalg.norm(axis), (np.trace(d) - 1) / 2)))
    return worst


def centred(f, pp, R):
    """The cameras with their principal points folded into the rotations: (f, zeros, C R), C the
    least rotation that takes the principal point's ray (-px / f, -py / f, 1) to the z axis."""
    out = []
    for fc, p, r in zip(f, pp, R):
        ray = np.array([-p[0] / fc, -p[1] / fc, 1.0])
        ray /= np.linalg.norm(ray)
        axis = np.cross(ray, [0, 0, 1.0])
        sin = np.linalg.norm(axis)
        out.append((rodrigues(axis / sin * np.arctan2(sin, ray[2])) if sin > 0 else np.eye(3)) @ r)
    return np.array(f, np.float64), np.zeros((len(f), 2)), np.stack(out)
