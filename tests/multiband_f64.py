"""A float64 restatement of the multiband blend (stitcher.py:185-241), test-side only.

``blur_f64`` and ``multiband_f64`` follow the reference's documented behaviour in float64: the
Gaussian of every level uses exactly the float32 taps the kernels use (``engine.gaussian_taps``,
held in float64), the border is REFLECT_101 (``scipy.ndimage``'s "mirror", which repeats the
reflection on planes narrower than the radius), ownership is the first maximum of the warped
alphas, every level blurs the ORIGINAL warped patch with the sharp ownership mask as alpha, level
k's tile carries G_k's alpha (the last level G_{L-2} itself, with G_{L-2}'s alpha), each level adds
``layer / wsum`` with ``wsum == 0 -> 1`` and the ``allmask`` zeroing, and the sum is clipped to
[0, 1] - the form of the oracle's ``float_out`` and of the kernels' ``want_float`` output, which
are both taken AFTER the clip (pano_oracle.c, ``orc_multiband_blend``; blend.hip,
``multiband_compose_kernel``).  Clipping is 1-Lipschitz, so a bound on the unclipped error holds
for the clipped one.

Error scale and bound
---------------------
u = 2^-24 (float32 unit roundoff).  Every operand of the blur is non-negative (colours, sharp
alphas, taps), so a blurred value B = sum_j t_j sum_i t_i x_ij is its own sum of absolute values,
and the per-pixel error scale of a blurred plane is ``s = B + F / u``.

F is the absolute floor of the matrix-core blur's operand representation (blur_mfma.hip): an
operand v is held as hi = f16(v S), lo = f16(v S - hi) at a power-of-two pre-scale S.  Where lo
(or hi) falls below float16's smallest normal 2^-14 it is a subnormal with spacing 2^-24, so the
pair represents v to within 2^-25 / S absolutely (and to 2^-22 |v| relatively where lo is normal).
With S = MB_TAP_SCALE = 2^8 for the taps, MB_IN_SCALE = 2^11 for the inputs and, for the
intermediate, MB_IN_SCALE again (the row pass's product is brought back by MB_MID_SCALE before its
split), one pass of n taps over data bounded by X has an absolute representation error of at
most  n X 2^-33  (taps)  +  2^-36  (data, the taps summing to 1).  Two passes:

    F = 2 (n X 2^-33 + 2^-36)                         (``blur_floor``)

- 2.7e-8 at n = 117 taps and X = 1, under half a u.  The vector-ALU blur (blur.hip) multiplies in
float32 and has no floor; F only loosens its bound.

For the mosaic the scale is the first-order sensitivity to a relative perturbation of every
blurred operand, built from the truth's own terms as sums of absolute values:

    s = sum_l [ sum_i a_il (|x_il| + |x_i,l+1|) + |c_l| sum_i a_il ] / wsum_l   (+ floor terms)

over the levels with wsum_l > 0 inside allmask (a = blurred alpha, x = blurred colour, x_i0 the
warped colour, c_l = layer_l / wsum_l).  The floor terms are the same expression with the relative
perturbations replaced by F: (sum_i (2 F_x a_il + F_a |x_il - x_i,l+1|) + |c_l| n_l F_a) / wsum_l,
divided by u.  A relative error eps on every blurred operand moves c_l by at most
eps (2 sum_i a (|x_l| + |x_l+1|) + |c_l| sum_i a) / wsum_l, i.e. by at most 2 eps s.

The normalised error is e(p) = |got - truth| / (u s(p)).  Its bound E (``bound``) counts the
roundings a blurred value goes through, taken one per operation at most u times the magnitude it
rounds (all magnitudes are bounded by the sums of absolute values that make up s), and counts a
sum as its mean-square rounding, not its worst case:

- the operand split (kernels): an operand's pair misses it by <= 2^-22 relative (hi is within
  2^-11 of v, lo rounds that remainder to 11 bits), and the dropped lo*lo product is <= 2^-22 of
  the product: 3 * 2^-22 = 12 u per pass on the (non-negative) sum, 24 u for the two passes;
- the float32 accumulation of a pass of n taps.  Round-to-nearest errors of the partial sums are
  independent with zero mean and variance <= (u S_k)^2 / 3 for a partial sum S_k <= B; their sum
  has a standard deviation <= u B sqrt(n / 3).  Across the ~10^7 values a suite compares, 6
  standard deviations (a two-sided tail of 2e-9 per value under a normal law) are not exceeded:
  6 sqrt(n / 3) u B per pass, where the kernels sum in fewer, longer steps (16-product MFMA
  blocks) and the oracle in n steps - the oracle's count is the larger and is the one taken;
- the two passes: 24 u + 12 sqrt(n / 3) u relative on a blurred value;
- the collapse: the difference x_l - x_l+1, the product with a, the sum over records, the sum
  over records of the alphas, the division and the sum over levels: at most (4 + m + L) u in
  units of s, for m overlapping records.

A blurred plane therefore meets  e <= E_plane(n) = 24 + 12 sqrt(n / 3),  and a mosaic value
e <= E(n_max, L, m) = 2 E_plane(n_max) + 4 + m + L with n_max the widest level's aperture.
"""
import numpy as np
from scipy.ndimage import correlate1d

from pano360_amd import engine

U = 2.0 ** -24

MB_IN_SCALE = 2.0 ** 11          # blur_mfma.hip
MB_TAP_SCALE = 2.0 ** 8
MB_MID_SCALE = 2.0 ** -8
F16_SUB_HALF = 2.0 ** -25        # half the spacing of float16 subnormals


def level_taps(sigma):
    """The float32 taps the kernels use for one level, held in float64."""
    return engine.gaussian_taps(engine.gaussian_ksize(sigma), sigma).astype(np.float64)


def blur_f64(plane, sigma):
    """Separable Gaussian of ``plane`` ([h][w] or [h][w][c]) in float64, REFLECT_101 border."""
    t = level_taps(sigma)
    out = correlate1d(np.asarray(plane, np.float64), t, axis=1, mode="mirror")
    return correlate1d(out, t, axis=0, mode="mirror")


def blur_floor(ntaps, xmax=1.0):
    """F: the absolute floor of the split-float16 operands over the two passes (docstring)."""
    mid_scale = MB_IN_SCALE * MB_TAP_SCALE * MB_MID_SCALE          # the intermediate's pre-scale
    per_pass = ntaps * xmax * F16_SUB_HALF / MB_TAP_SCALE + F16_SUB_HALF / min(MB_IN_SCALE, mid_scale)
    return 2.0 * per_pass


def plane_bound(ntaps):
    """E_plane: the bound on e of a blurred plane (docstring)."""
    return 24.0 + 12.0 * np.sqrt(ntaps / 3.0)


def bound(ntaps, n_levels, overlap):
    """E: the bound on e of a mosaic value (docstring); ``overlap`` = most records on a pixel."""
    return 2.0 * plane_bound(ntaps) + 4.0 + overlap + n_levels


def max_taps(n_levels):
    return max([engine.gaussian_ksize(s) for s in engine.level_sigmas(n_levels)] or [1])


def ownership_f64(patches, shape):
    """First-maximum argmax of the warped alphas, -1 where every alpha is 0 (stitcher.py:196-204)."""
    best = np.zeros(shape, np.float32)
    owner = np.full(shape, -1, np.int32)
    for i, (warped, _, ir) in enumerate(patches):
        a = warped[..., 3]
        b = best[ir]
        upd = a > b
        owner[ir][upd] = i
        b[upd] = a[upd]
    return owner


def multiband_f64(patches, shape, n_levels, xmax=None):
    """The multiband blend of the oracle's float32 warped ``patches`` ((warped, mask, irange)
    triples, not modified) in float64.  Returns (mosaic [H][W][3] clipped to [0, 1], s [H][W][3],
    overlap): the truth in the form of ``float_out``, its error scale, and the most records that
    meet one pixel."""
    H, W = shape
    owner = ownership_f64(patches, shape)
    allmask = np.zeros(shape, bool)
    for warped, mask, ir in patches:
        allmask[ir] |= ~np.asarray(mask, bool)
    sig = engine.level_sigmas(n_levels)
    L = n_levels
    if xmax is None:
        xmax = max([1.0] + [float(np.abs(p[0][..., :3]).max()) for p in patches if p[0].size])
    floor = blur_floor(max_taps(n_levels), xmax) if L > 1 else 0.0
    layer = np.zeros((L, H, W, 3))
    wsum = np.zeros((L, H, W))
    sabs = np.zeros((L, H, W, 3))          # sum_i a (|x_l| + |x_l+1|)
    fabs = np.zeros((L, H, W, 3))          # sum_i (2 F a + F |x_l - x_l+1|)
    count = np.zeros((L, H, W))            # records with a > 0
    cover = np.zeros(shape, np.int32)
    for i, (warped, mask, ir) in enumerate(patches):
        rgba = np.asarray(warped, np.float64).copy()
        rgba[..., 3] = owner[ir] == i
        cover[ir] += not np.asarray(mask, bool).all()     # (a record masked everywhere adds nothing)
        xs = [rgba] + [blur_f64(rgba, s) for s in sig]
        for lvl in range(L):
            if lvl < L - 1:
                x_hi, x_lo, a = xs[lvl][..., :3], xs[lvl + 1][..., :3], xs[lvl + 1][..., 3]
                tile = x_hi - x_lo
                mag = np.abs(x_hi) + np.abs(x_lo)
            else:
                tile, a = xs[lvl][..., :3], xs[lvl][..., 3]
                mag = np.abs(tile)
            layer[lvl][ir] += tile * a[..., None]
            wsum[lvl][ir] += a
            sabs[lvl][ir] += mag * a[..., None]
            if floor:
                fabs[lvl][ir] += floor * (2.0 * a[..., None] + np.abs(tile))
            count[lvl][ir] += a > 0
    mosaic = np.zeros((H, W, 3))
    s = np.zeros((H, W, 3))
    for lvl in range(L):
        ws = np.where(wsum[lvl] == 0, 1.0, wsum[lvl])[..., None]
        lay = np.where(allmask[..., None], layer[lvl], 0.0)
        c = lay / ws
        mosaic += c
        live = (allmask & (wsum[lvl] > 0))[..., None]
        term = (sabs[lvl] + np.abs(c) * wsum[lvl][..., None]) / ws
        term += (fabs[lvl] + np.abs(c) * (count[lvl] * floor)[..., None]) / ws / U
        s += np.where(live, term, 0.0)
    return np.clip(mosaic, 0.0, 1.0), s, int(cover.max()) if cover.size else 0


def normalised_error(got, truth, s):
    """e(p) = |got - truth| / (u s(p)); pixels with s = 0 (outside allmask: the truth is an exact
    0 there) count as e = 0 when got is exactly the truth and infinity otherwise."""
    diff = np.abs(np.asarray(got, np.float64) - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(s > 0, diff / (U * s), np.where(diff == 0, 0.0, np.inf))
    return e


def plane_error(got, truth, ntaps, xmax=1.0):
    """e of a blurred plane against its float64 truth: s = truth + F / u."""
    s = np.asarray(truth, np.float64) + blur_floor(ntaps, xmax) / U
    return np.abs(np.asarray(got, np.float64) - truth) / (U * s)
