"""A float64 restatement of the SIFT front end (OpenCV's sift.cpp with the SIFT_create() defaults;
scalespace.hip, sift.hip), stage by stage and test-side only, parameterised by the layers per
octave.  Every stage takes float32 inputs identical to what the kernel read - the kernel's own
previous layer, its own DoG planes, keypoint records built on the host - so a comparison judges
that stage's arithmetic alone.  Each item gets an error bound from the float32 arithmetic of the
stage; a discrete outcome (an extremum kept, a Newton move, a histogram bin, a peak) is *decided*
when the quantity that decides it lies farther than that bound from the threshold, and a correct
float32 implementation - the kernel, or the float32 oracle under oracle/ - must then reach the
same outcome.  Items with an outcome inside its margin are *undecided*: they may come or go.

u = 2^-24 (float32 unit roundoff) throughout; "a rounding" is at most u times the magnitude it
rounds, and every bound below counts one per float32 operation (fused or not).

Scale step (``step_f64``)
-------------------------
Layer i = the separable REFLECT_101 correlation of layer i-1 with the float32 taps the kernels use
(``features._step_taps``, cv::getGaussianKernel; SciPy's "mirror" mode, which repeats the
reflection on planes narrower than the radius).  Taps and grey levels are non-negative, so the
blurred value B is its own sum of absolute values and the error scale of a pixel is s = B.  A pass
of n taps makes at most 2n roundings of partial sums <= B (a product and an add per tap in the
oracle's NumPy form; one FMA per tap in the kernel's); the column pass carries the row pass's
relative error through taps summing to 1.  So e = |got - B| / (u B) <= E_step(n) = 4n (worst
case, no statistics).  DoG_{i-1} = float32(G_i - G_{i-1}) of the stored layers is exact to check.

Extrema
-------
The candidates are exact: comparisons of identical float32 values against the integer
floor(0.5 * 0.04 / n_layers * 255); no float64 is needed.

Refinement (``refine_f64``, adjustLocalExtrema)
-----------------------------------------------
Newton steps in float64 on the float32 DoG samples, with the float32 scales of sift.cpp
(1/255, its half and quarter).  The float32 derivatives are off by at most 2u (first), 3u
(second) and 4u (cross) times the sums of absolute values of their terms (``gabs``, ``Habs``).
The 3 x 3 solve by LU with partial pivoting has a backward error of at most gamma_3 |L||U| <=
3.1 u x 3 x 4 max|H| (growth <= 4 for 3 x 3), taken as 40 u m with m = max Habs.  First order:

    |dx| <= 2 |H^-1| ((4u Habs + 40u m) |x| + 2u gabs + u |g|)

(the factor 2 for the second-order terms).  Every decision of a step is measured against it:
each rint move and the |x| < 0.5 exit (both flip only at a half-integer, so a component within
dx of one leaves the keypoint undecided), and the pivot test, |p_k| against 10 FLT_EPSILON with
the pivots p_k of the same elimination in float64, decided when no pivot lies within 40 u m of
the threshold.  The contrast |contr| n_layers against 0.04 with contr = D/255 + g.x/2 and the edge
test tr^2 10 against 121 det (det <= 0 first) are decided outside their first-order bounds
(``_contrast_edge``).  A keypoint with any decision inside its margin is undecided.

The pivot threshold is the project's choice, not OpenCV's behaviour.  sift.cpp solves
``Matx33f H; Vec3f X = H.solve(dD, DECOMP_LU)``: a 3 x 3 matrix with one right-hand side, which
OpenCV's matx headers (2.4 through 4.x, as far as is known; OpenCV is not pinned) hand to the
``Matx_FastSolveOp<float, 3, 1>`` specialisation - Cramer's rule, singular only when the
determinant is exactly 0.  sift.hip's ``solve3`` restates instead the float LU that DECOMP_LU
names elsewhere, ``hal::LU32f`` (OpenCV's ``LUImpl`` with eps = FLT_EPSILON * 10: Gaussian
elimination with partial pivoting that gives up when the largest remaining pivot is below eps,
after which ``Matx::solve`` returns zeros).  oracle/sift_oracle.py's ``_solve3`` now follows the
kernel, so that the kernel, the oracle and this restatement judge one operation.

Keypoint values: x, y = (c + xc) 2^o, bound 2^o (dx_c + 2u |c + xc|); size = sigma 2^((layer +
xi) / n) 2^(o+1), bound size (ln 2 / n dx_i + 8u); response = |contr|, bound its contrast bound.

Orientation (``orientation_f64``, calcOrientationHist)
-----------------------------------------------------
A 36-bin histogram in float64 of w |grad| at bin rint(fastAtan2 / 10), with the float64
evaluation of ``cv::fastAtan2``'s polynomial (its float32 coefficients; the operation as OpenCV
defines it, not atan2).  The angle of a sample is off in float32 by at most 1000 u degrees (the
quotient by a reciprocal of 1 ulp, four FMAs of a polynomial worth 45 degrees, the quadrant
folds of 360) - plus the polynomial's own jump of |2 p(1) - 90| = 0.0062 degrees at the branch
switch |dx| = |dy|, where float32 differences may fall on the other side.  A sample whose bin
value is within that of a half-integer is ambiguous: its vote is uncertain in both bins.  A
vote's magnitude is off by at most 10 u relative (exp, sqrt, the product) plus half the kernel's
fixed-point unit 2^-20.  So each bin is an interval; the [1 4 6 4 1] / 16 smoothing (positive
weights) carries intervals; a bin is a decided peak when its interval lies above both
neighbours' and above 0.8 times the largest upper end, decided not a peak when it cannot be; the
parabola's angle is taken at the truth with the spread of its values over the corners of the
three intervals as its bound (+ 1e-3 degrees of float32 evaluation).

Descriptor (``descriptor_f64``, calcSIFTDescriptor)
--------------------------------------------------
The real-valued 128-vector before rounding: trilinear votes of w |grad| into 4 x 4 x 8 bins, the
clip at 0.2 ||v|| and the scale 512 / ||v'||.  The trilinear split is continuous in (rbin, cbin,
obin): at an integer the vote is wholly in one bin.  The window cut-offs -1 < rbin, cbin < 4 fall
where the votes that would cross them weigh 0 in the four kept cells (the two outer cells of each
axis are padding, never read), the orientation wraps modulo 8 bins, and the window's radius
rint(3 scl sqrt2 5 / 2) covers every sample inside the cut-off whichever way it rounds (the clip
to the plane's diagonal never cuts an in-image sample).  Clip, norm and scale are continuous.
fastAtan2's jump at |dx| = |dy| is bounded as above.  So the only discontinuity left is the
final rint: a correct float32 result is round(v) wherever v lies more than its error scale
delta from a half-integer, and everywhere |got - clip(v, 0, 255)| <= 0.5 + delta.

delta collects, per sample and per bin it votes into, the magnitude times its relative error
(10 u + the exp argument's error) and times the errors of its three bin coordinates (each
trilinear weight has derivative at most 1 in each coordinate), plus half the kernel's
fixed-point unit 2^-kbits per vote (kbits chosen per keypoint in sift.hip).  The clip and the
normalisation carry it: delta_out = 512 (dv'_i / |v'| + v'_i |dv'| / |v'|^2) + 30 u out_i, with
dv' = dv + 0.2 |dv| on clipped entries.
"""
import numpy as np
from scipy.ndimage import correlate1d

U = 2.0 ** -24
F = np.float32
FLT_EPSILON = float(np.finfo(np.float32).eps)
PIVOT_EPS = float(F(FLT_EPSILON * 10))
CONTRAST_THR = 0.04
EDGE_THR = 10.0
SIGMA = 1.6
BORDER = 5
MAX_STEPS = 5
IMG_SCALE = float(F(1.0 / 255.0))
DERIV_SCALE = float(F(F(1.0 / 255.0) * F(0.5)))
CROSS_SCALE = float(F(F(1.0 / 255.0) * F(0.25)))

_P = [float(F(v * (180 / np.pi))) for v in (0.9997878412794807, -0.3258083974640975,
                                             0.1555786518463281, -0.04432655554792128)]
ATAN_JUMP = abs(2.0 * sum(_P) - 90.0)          # fastAtan2's step at |dx| = |dy|
ATAN_ERR = 1000.0 * U                           # degrees, away from the switch


# --------------------------------------------------------------------------- scale step
def step_f64(plane, taps):
    """One Gaussian step: the separable REFLECT_101 correlation with the float32 ``taps``."""
    t = np.asarray(taps, np.float32).astype(np.float64)
    out = correlate1d(np.asarray(plane, np.float64), t, axis=1, mode="mirror")
    return correlate1d(out, t, axis=0, mode="mirror")


def step_bound(ntaps):
    """E_step: the bound on e of one scale step (docstring)."""
    return 4.0 * ntaps


def step_error(got, truth):
    """e = |got - B| / (u B); B = 0 (an all-zero window) counts as 0 only when got is 0 too."""
    diff = np.abs(np.asarray(got, np.float64) - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(truth > 0, diff / (U * truth), np.where(diff == 0, 0.0, np.inf))


def up2_f64(grey):
    """createInitialImage's 2x INTER_LINEAR upsampling of the integer grey image in float64 (the
    weights 1/4, 3/4 of oracle/sift_pyramid.py, exact in float32).  The kernel's float32 form
    rounds at most four times (a sum per pass, a product and a sum in the second) values no larger
    than the non-negative result: its base is within 4 u B of this one, and a step over it within
    ``step_bound(n) + 4`` (the taps sum to 1)."""
    import sift_pyramid as sp
    g = np.asarray(grey, np.float64)
    h, w = g.shape
    x0, x1, a0, a1 = sp._up2_taps(w)
    y0, y1, b0, b1 = sp._up2_taps(h)
    rows = g[:, x0] * a0.astype(np.float64) + g[:, x1] * a1.astype(np.float64)
    return rows[y0] * b0.astype(np.float64)[:, None] + rows[y1] * b1.astype(np.float64)[:, None]


# --------------------------------------------------------------------------- extrema
def threshold(n_layers):
    return int(np.floor(0.5 * CONTRAST_THR / n_layers * 255))


def extrema(dog, n_layers):
    """findScaleSpaceExtrema's candidates of one octave's DoG stack [n_layers + 2][R][C]:
    int array [K][3] of (layer, r, c), exact."""
    dog = np.asarray(dog, np.float32)
    L, R, C = dog.shape
    assert L == n_layers + 2
    if R <= 2 * BORDER or C <= 2 * BORDER:
        return np.zeros((0, 3), np.int64)
    thr = np.float32(threshold(n_layers))
    out = []
    for i in range(1, n_layers + 1):
        cur = dog[i, BORDER:R - BORDER, BORDER:C - BORDER]
        hi = lo = None
        for dl in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    v = dog[i + dl, BORDER + dy:R - BORDER + dy, BORDER + dx:C - BORDER + dx]
                    hi = v if hi is None else np.maximum(hi, v)
                    lo = v if lo is None else np.minimum(lo, v)
        cand = (np.abs(cur) > thr) & (((cur > 0) & (cur >= hi)) | ((cur < 0) & (cur <= lo)))
        rr, cc = np.nonzero(cand)
        out.append(np.stack([np.full(len(rr), i), rr + BORDER, cc + BORDER], axis=1))
    return np.concatenate(out).astype(np.int64)


# --------------------------------------------------------------------------- refinement
def _derivs(D, l, r, c):
    """g, H and their sums of absolute values (float64 [K][3], [K][3][3]) at (l, r, c)."""
    def a(dl, dr, dc):
        return D[l + dl, r + dr, c + dc]
    v = a(0, 0, 0)
    first = [(a(0, 0, 1), a(0, 0, -1)), (a(0, 1, 0), a(0, -1, 0)), (a(1, 0, 0), a(-1, 0, 0))]
    g = np.stack([(p - q) * DERIV_SCALE for p, q in first], 1)
    gabs = np.stack([(np.abs(p) + np.abs(q)) * DERIV_SCALE for p, q in first], 1)
    sec = [(p + q - 2 * v) * IMG_SCALE for p, q in first]
    sec_abs = [(np.abs(p) + np.abs(q) + 2 * np.abs(v)) * IMG_SCALE for p, q in first]

    def cross(p, q, s, t):
        return (p - q - s + t) * CROSS_SCALE, (np.abs(p) + np.abs(q) + np.abs(s) + np.abs(t)) * CROSS_SCALE
    dxy, axy = cross(a(0, 1, 1), a(0, 1, -1), a(0, -1, 1), a(0, -1, -1))
    dxs, axs = cross(a(1, 0, 1), a(1, 0, -1), a(-1, 0, 1), a(-1, 0, -1))
    dys, ays = cross(a(1, 1, 0), a(1, -1, 0), a(-1, 1, 0), a(-1, -1, 0))
    H = np.stack([np.stack([sec[0], dxy, dxs], 1), np.stack([dxy, sec[1], dys], 1),
                  np.stack([dxs, dys, sec[2]], 1)], 1)
    Habs = np.stack([np.stack([sec_abs[0], axy, axs], 1), np.stack([axy, sec_abs[1], ays], 1),
                     np.stack([axs, ays, sec_abs[2]], 1)], 1)
    return v, g, gabs, H, Habs


def lu_pivots(H):
    """The pivots of Gaussian elimination with partial pivoting, float64 [K][3]."""
    a = np.array(H, np.float64)
    K = len(a)
    ar = np.arange(K)
    piv = np.zeros((K, 3))
    for i in range(3):
        k = i + np.argmax(np.abs(a[:, i:, i]), axis=1)
        row = a[ar, i].copy()
        a[ar, i] = a[ar, k]
        a[ar, k] = row
        p = a[:, i, i]
        piv[:, i] = p
        safe = np.where(p == 0, 1.0, p)
        for j in range(i + 1, 3):
            a[:, j, :] -= (a[:, j, i] / safe)[:, None] * a[:, i, :]
    return piv


def _solve(H, Habs, g, gabs):
    """(solution, its bound, singular, pivot decided) of H x = g as sift.cpp's solve (zeros when
    a pivot is below 10 FLT_EPSILON)."""
    m = Habs.reshape(len(H), -1).max(axis=1)
    piv = np.abs(lu_pivots(H))
    singular = (piv < PIVOT_EPS).any(axis=1)
    piv_ok = (np.abs(piv - PIVOT_EPS) > 40 * U * m[:, None]).all(axis=1)
    x = np.zeros_like(g)
    dx = np.zeros_like(g)
    ok = ~singular
    if ok.any():
        Hs = H[ok]
        x[ok] = np.linalg.solve(Hs, g[ok][..., None])[..., 0]
        inv = np.abs(np.linalg.inv(Hs))
        dH = 4 * U * Habs[ok] + 40 * U * m[ok][:, None, None]
        rhs = np.einsum("kij,kj->ki", dH, np.abs(x[ok])) + 2 * U * gabs[ok] + U * np.abs(g[ok])
        dx[ok] = 2 * np.einsum("kij,kj->ki", inv, rhs) + 2 * U * np.abs(x[ok])
    return x, dx, singular, piv_ok


def _near_half(x, dx):
    """True where x lies within dx of a half-integer (rint and |x| < 0.5 can go either way)."""
    return np.abs(np.abs(x - np.floor(x)) - 0.5) <= dx


def _contrast_edge(v, g, H, Habs, gabs, x, dx, n_layers):
    """contr, its bound, contrast kept, edge kept, and whether all three decisions are decided."""
    t = (g * x).sum(1)
    contr = v * IMG_SCALE + 0.5 * t
    dcontr = (2 * U * np.abs(v * IMG_SCALE) + 0.5 * ((np.abs(g) * dx).sum(1) +
              (2 * U * gabs * np.abs(x)).sum(1)) + 4 * U * (np.abs(g * x)).sum(1) + U * np.abs(contr))
    q = np.abs(contr) * n_layers - CONTRAST_THR
    keep_c = q >= 0
    dec_c = np.abs(q) > n_layers * dcontr + U * CONTRAST_THR
    dxx, dyy, dxy = H[:, 0, 0], H[:, 1, 1], H[:, 0, 1]
    exx, eyy, exy = 4 * U * Habs[:, 0, 0], 4 * U * Habs[:, 1, 1], 4 * U * Habs[:, 0, 1]
    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
    dtr = exx + eyy + U * np.abs(tr)
    ddet = (np.abs(dyy) * exx + np.abs(dxx) * eyy + 2 * np.abs(dxy) * exy +
            3 * U * (np.abs(dxx * dyy) + dxy * dxy))
    f = tr * tr * EDGE_THR - (EDGE_THR + 1) ** 2 * det
    df = 2 * EDGE_THR * np.abs(tr) * dtr + (EDGE_THR + 1) ** 2 * ddet + \
        4 * U * (EDGE_THR * tr * tr + (EDGE_THR + 1) ** 2 * np.abs(det))
    keep_e = (det > 0) & (f < 0)
    dec_e = (np.abs(det) > ddet) & ((det <= 0) | (np.abs(f) > df))
    return contr, dcontr, keep_c, keep_c & keep_e, dec_c & (~keep_c | dec_e)


def refine_f64(dog, octv, cands, n_layers, sigma=SIGMA):
    """adjustLocalExtrema and the keypoint record of every candidate (layer, r, c) of ``extrema``
    on the float32 DoG stack of octave ``octv``.  Returns a dict of arrays over the candidates:
    ``kept``, ``decided``, final ``layer`` / ``r`` / ``c``, ``x`` / ``y`` / ``size`` /
    ``response`` with their bounds ``dx`` / ``dy`` / ``dsize`` / ``dresp``, ``octave`` (the packed
    word), ``oct_decided`` (its third byte, rint((xi + 0.5) 255), is decided) and ``path``
    ([K][6][3]: (layer, r, c) after each Newton step)."""
    D = np.asarray(dog, np.float32).astype(np.float64)
    _, R, C = D.shape
    cands = np.asarray(cands, np.int64).reshape(-1, 3)
    K = len(cands)
    layer, r, c = (cands[:, k].copy() for k in range(3))
    alive = np.ones(K, bool)
    path = np.repeat(cands[:, None, :], MAX_STEPS + 1, axis=1)      # (layer, r, c) after each step
    done = np.zeros(K, bool)
    decided = np.ones(K, bool)
    x = np.zeros((K, 3))
    dx = np.zeros((K, 3))
    big = float(F(2147483647 // 3))
    for step in range(MAX_STEPS):
        act = np.nonzero(alive & ~done)[0]
        if not len(act):
            break
        _, g, gabs, H, Habs = _derivs(D, layer[act], r[act], c[act])
        sol, dsol, _, piv_ok = _solve(H, Habs, g, gabs)
        xs, ds = -sol, dsol
        x[act], dx[act] = xs, ds
        decided[act] &= piv_ok & ~_near_half(xs, ds).any(1)
        conv = (np.abs(xs) < 0.5).all(1)
        done[act[conv]] = True
        mv = act[~conv]
        xm = xs[~conv]
        huge = (np.abs(xm) > big).any(1)
        alive[mv[huge]] = False
        mv, xm = mv[~huge], xm[~huge]
        c[mv] += np.rint(xm[:, 0]).astype(np.int64)
        r[mv] += np.rint(xm[:, 1]).astype(np.int64)
        layer[mv] += np.rint(xm[:, 2]).astype(np.int64)
        path[mv, step + 1:] = np.stack([layer[mv], r[mv], c[mv]], 1)[:, None, :]
        out = ((layer[mv] < 1) | (layer[mv] > n_layers) | (c[mv] < BORDER) | (c[mv] >= C - BORDER) |
               (r[mv] < BORDER) | (r[mv] >= R - BORDER))
        alive[mv[out]] = False
    alive &= done
    res = dict(kept=np.zeros(K, bool), decided=decided, layer=layer, r=r, c=c, path=path,
               x=np.zeros(K), y=np.zeros(K), size=np.zeros(K), response=np.zeros(K),
               dx=np.zeros(K), dy=np.zeros(K), dsize=np.zeros(K), dresp=np.zeros(K),
               octave=np.zeros(K, np.int64), oct_decided=np.ones(K, bool))
    idx = np.nonzero(alive)[0]
    if len(idx):
        v, g, gabs, H, Habs = _derivs(D, layer[idx], r[idx], c[idx])
        xa, da = x[idx], dx[idx]
        contr, dcontr, _, keep, dec = _contrast_edge(v, g, H, Habs, gabs, xa, da, n_layers)
        res["decided"][idx] &= dec
        k = idx[keep]
        xa, da, contr, dcontr = xa[keep], da[keep], contr[keep], dcontr[keep]
        res["kept"][k] = True
        scale = float(1 << octv)
        res["x"][k] = (c[k] + xa[:, 0]) * scale
        res["y"][k] = (r[k] + xa[:, 1]) * scale
        res["dx"][k] = scale * (da[:, 0] + 2 * U * np.abs(c[k] + xa[:, 0]))
        res["dy"][k] = scale * (da[:, 1] + 2 * U * np.abs(r[k] + xa[:, 1]))
        size = sigma * 2.0 ** ((layer[k] + xa[:, 2]) / n_layers) * scale * 2
        res["size"][k] = size
        res["dsize"][k] = size * (np.log(2) / n_layers * da[:, 2] + 8 * U)
        res["response"][k] = np.abs(contr)
        res["dresp"][k] = dcontr
        q = (xa[:, 2] + 0.5) * 255
        res["octave"][k] = octv + (layer[k] << 8) + (np.rint(q).astype(np.int64) << 16)
        res["oct_decided"][k] = ~_near_half(q, 255 * da[:, 2] + 2 * U * np.abs(q))
    return res


# --------------------------------------------------------------------------- angles
def fast_atan2_f64(y, x):
    """cv::fastAtan2's polynomial (its float32 coefficients) evaluated in float64, degrees."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    ax, ay = np.abs(x), np.abs(y)
    swap = ax < ay
    num, den = np.where(swap, ax, ay), np.where(swap, ay, ax) + 2.220446049250313e-16
    cq = num / den
    c2 = cq * cq
    a = (((_P[3] * c2 + _P[2]) * c2 + _P[1]) * c2 + _P[0]) * cq
    a = np.where(swap, 90.0 - a, a)
    a = np.where(x < 0, 180.0 - a, a)
    return np.where(y < 0, 360.0 - a, a)


def atan_error(dy, dx):
    """The float32 error scale of a sample's fastAtan2 (degrees): the jump where the float32
    differences may fall on the other side of |dx| = |dy|."""
    ax, ay = np.abs(dx), np.abs(dy)
    near = np.abs(ax - ay) <= 2 * U * (ax + ay)
    return ATAN_ERR + np.where(near, ATAN_JUMP, 0.0)


def _window(img, r, c, radius):
    """(i, j, dx, dy) of the window samples strictly inside the plane."""
    rows, cols = img.shape
    i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    i, j = i.ravel(), j.ravel()
    y, x = r + i, c + j
    ok = (y > 0) & (y < rows - 1) & (x > 0) & (x < cols - 1)
    i, j, y, x = i[ok], j[ok], y[ok], x[ok]
    im = np.asarray(img, np.float32).astype(np.float64)
    return i, j, im[y, x + 1] - im[y, x - 1], im[y - 1, x] - im[y + 1, x]


def orientation_hist_f64(img, r, c, size, octv):
    """calcOrientationHist's raw 36-bin histogram (before smoothing) of a candidate (octave
    coordinates r, c; record size) in float64, and each bin's float32 error scale (docstring)."""
    n = 36
    scl = float(F(F(F(size) * F(0.5)) / F(1 << octv)))
    radius = int(np.rint(F(F(4.5) * F(scl))))
    sig = float(F(F(1.5) * F(scl)))
    i, j, dx, dy = _window(img, r, c, radius)
    w = np.exp((i * i + j * j) * (-1.0 / (2.0 * sig * sig)))
    mag = np.hypot(dx, dy) * w
    b = fast_atan2_f64(dy, dx) / 10.0
    db = atan_error(dy, dx) / 10.0 + 4 * U * b
    b0 = np.rint(b).astype(np.int64) % n
    amb = _near_half(b, db)
    hist = np.zeros(n)
    err = np.zeros(n)
    np.add.at(hist, b0, mag)
    np.add.at(err, b0, mag * 10 * U + 2.0 ** -20)
    alt = np.where(b - np.floor(b) < 0.5, np.ceil(b), np.floor(b)).astype(np.int64) % n
    np.add.at(err, b0[amb], mag[amb])
    np.add.at(err, alt[amb], mag[amb])
    return hist, err


def orientation_f64(img, r, c, size, octv):
    """calcOrientationHist of a candidate and its peaks: a list of (angle, bound, decided) per bin
    that is or may be a peak."""
    n = 36
    hist, err = orientation_hist_f64(img, r, c, size, octv)

    def smooth(h):
        return (np.roll(h, 2) + np.roll(h, -2)) / 16 + (np.roll(h, 1) + np.roll(h, -1)) * 4 / 16 + h * 6 / 16
    S, dS = smooth(hist), smooth(err) + 8 * U * smooth(hist)
    lo, hi = S - dS, S + dS
    out = []
    for k in range(n):
        l, rr = (k - 1) % n, (k + 1) % n
        yes = lo[k] > hi[l] and lo[k] > hi[rr] and lo[k] >= 0.8 * hi.max()
        no = hi[k] <= lo[l] or hi[k] <= lo[rr] or hi[k] < 0.8 * lo.max()
        if no:
            continue
        vals = []
        for hl in (lo[l], hi[l]):
            for hk in (lo[k], hi[k]):
                for hr in (lo[rr], hi[rr]):
                    den = hl - 2 * hk + hr
                    vals.append(0.5 * (hl - hr) / den if den < 0 else np.nan)
        den = S[l] - 2 * S[k] + S[rr]
        off = 0.5 * (S[l] - S[rr]) / den if den < 0 else 0.0
        spread = np.nanmax(np.abs(np.array(vals) - off)) if np.isfinite(vals).all() else 1.0
        angle = (360.0 - 10.0 * ((k + off) % n)) % 360.0
        out.append((angle, 10.0 * spread + 1e-3, bool(yes)))
    return out


# --------------------------------------------------------------------------- descriptor
def unpack_octave(packed):
    octave, layer = packed & 255, (packed >> 8) & 255
    if octave >= 128:
        octave |= -128
    return octave, layer


def descriptor_f64(img, kx, ky, ksize, kangle, packed):
    """calcSIFTDescriptor of a keypoint record as the describe kernel reads it (full-resolution
    x, y, size, angle after the first-octave adjustment; the packed octave word) on its Gaussian
    plane ``img``.  Returns (v [128] before rounding and saturation, delta [128])."""
    d, nb = 4, 8
    octave, _ = unpack_octave(int(packed))
    scale = 2.0 ** -octave
    px, py = int(np.rint(F(F(kx) * F(scale)))), int(np.rint(F(F(ky) * F(scale))))
    ori = F(F(360.0) - F(kangle))
    if abs(float(ori) - 360.0) < FLT_EPSILON:
        ori = F(0.0)
    ori = float(ori)
    scl = float(F(F(ksize) * F(scale)) * F(0.5))
    hw = 3.0 * scl
    radius = int(np.rint(F(F(F(F(3.0) * F(scl)) * F(1.4142135623730951)) * F(d + 1)) * F(0.5)))
    rows, cols = img.shape
    radius = min(radius, int(np.sqrt(float(cols) * cols + float(rows) * rows)))
    cos_t, sin_t = np.cos(np.deg2rad(ori)) / hw, np.sin(np.deg2rad(ori)) / hw
    i, j, dx, dy = _window(img, py, px, radius)
    c_rot, r_rot = j * cos_t - i * sin_t, j * sin_t + i * cos_t
    rbin, cbin = r_rot + d / 2 - 0.5, c_rot + d / 2 - 0.5
    ok = (rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d)
    i, j, dx, dy, c_rot, r_rot, rbin, cbin = (a[ok] for a in (i, j, dx, dy, c_rot, r_rot, rbin, cbin))
    arg = (c_rot * c_rot + r_rot * r_rot) * (-1.0 / (d * d * 0.5))
    mag = np.hypot(dx, dy) * np.exp(arg)
    ang = fast_atan2_f64(dy, dx)
    obin = (ang - ori) * (nb / 360.0)
    # errors of the bin coordinates and of the magnitude (docstring)
    dpos = (np.abs(i) + np.abs(j)) * 10 * U / hw + 2 * U * (np.abs(r_rot) + np.abs(c_rot) + 1)
    dob = atan_error(dy, dx) * (nb / 360.0) + 8 * U * (np.abs(obin) + 1)
    drel = 10 * U + 3 * U * np.abs(arg) + (2 * np.abs(c_rot) + 2 * np.abs(r_rot)) * dpos / 8
    evote = mag * (drel + 2 * dpos + dob + 10 * U)
    kbits = 31 - int(np.ceil(np.log2(F(F(36.0) * F(max(scl * scl, 1.0)) * F(361.0)))))
    kbits = min(max(kbits, 0), 24)
    unit = 2.0 ** -kbits
    r0, c0, o0 = np.floor(rbin).astype(np.int64), np.floor(cbin).astype(np.int64), np.floor(obin).astype(np.int64)
    fr, fc, fo = rbin - r0, cbin - c0, obin - o0
    o0 %= nb
    hist = np.zeros((d + 2, d + 2, nb + 2))
    herr = np.zeros_like(hist)
    for a_r, w_r in ((0, 1 - fr), (1, fr)):
        for a_c, w_c in ((0, 1 - fc), (1, fc)):
            for a_o, w_o in ((0, 1 - fo), (1, fo)):
                at = (r0 + 1 + a_r, c0 + 1 + a_c, o0 + a_o)
                np.add.at(hist, at, mag * w_r * w_c * w_o)
                np.add.at(herr, at, evote + 0.5 * unit)
    hist[:, :, 0] += hist[:, :, nb]
    hist[:, :, 1] += hist[:, :, nb + 1]
    herr[:, :, 0] += herr[:, :, nb]
    herr[:, :, 1] += herr[:, :, nb + 1]
    v = hist[1:d + 1, 1:d + 1, :nb].reshape(-1)
    dv = herr[1:d + 1, 1:d + 1, :nb].reshape(-1) + U * v
    nrm = np.sqrt((v * v).sum())
    dn = np.sqrt((dv * dv).sum())
    thr = 0.2 * nrm
    vp = np.minimum(v, thr)
    dvp = dv + np.where(v + dv >= thr - 0.2 * dn, 0.2 * dn + U * thr, 0.0)
    n2 = max(np.sqrt((vp * vp).sum()), FLT_EPSILON)
    dn2 = np.sqrt((dvp * dvp).sum())
    out = vp * (512.0 / n2)
    delta = 512.0 * (dvp / n2 + vp * dn2 / (n2 * n2)) + 30 * U * out
    return out, delta
