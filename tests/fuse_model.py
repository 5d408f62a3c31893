"""The contract of ``pano_fuse_u8`` (include/pano360.h) in NumPy: what tests/test_gpu_fuse.py
holds the device against, and what tests/test_fuse_host.py checks the properties of.

``raw_weights`` is stage A in a chosen dtype (float64 for truth, the float32 constants widened);
``fuse_from_raw`` runs stages B .. E in float32, one rounding per operation in the contract's
order, over ``cv2_shim.pyrDown`` / ``pyrUp`` (oracle/ is on the path through conftest.py).

Why the device's float32 raw weights may differ from the float64 ones by 2e-5 at most (the bound
of the GPU test, exponents (1, 1, 1)): every byte / 255 carries half an ulp, about 6e-8.
C = |lap| <= 4 is a sum of five terms of magnitude up to 4: an absolute error of at most about
32 ulp(1), 2e-6.  S <= 0.4714 (two channels at one end, one at the other) comes from squares of
differences below 1 and one square root: at most 5e-7 absolute.  The argument of exp is at most
3 * 0.25 / 0.08 = 9.4 in magnitude and carries about 5 ulp of relative error, so E has a relative
error of at most 9.4 * 5 * 6e-8 = 3e-6, 5e-6 with expf's own few ulp.  With C <= 4, S <= 0.4714
and E <= 1 the product's error is at most 2e-6 * 0.4714 + 4 * 5e-7 + 4 * 0.4714 * 5e-6 = 1.3e-5,
below 2e-5.  An exponent of 2 on C doubles C's relative error: twice the bound.
"""
import numpy as np

import cv2_shim

MAX_EXPOSURES = 8


def levels_for(h, w):
    return max(0, int(min(h, w)).bit_length() - 2)


def _power(v, e, dtype):
    """v^e as the contract has it: 1 takes v as it is, 0 leaves it out (None)."""
    if e == 1:
        return v
    if e == 0:
        return None
    return np.power(v, dtype(e)).astype(dtype)


def raw_weights(img, dtype=np.float64, params=(1.0, 1.0, 1.0)):
    """Stage A on one uint8 [h][w][3] BGR frame: W [h][w] in ``dtype``."""
    ft = dtype
    img = np.asarray(img)
    h, w = img.shape[:2]
    v = img.astype(ft) / ft(np.float32(255.0))
    B, G, R = v[..., 0], v[..., 1], v[..., 2]
    g = (ft(np.float32(0.114)) * B + ft(np.float32(0.587)) * G) + ft(np.float32(0.299)) * R
    xs, ys = np.arange(w), np.arange(h)
    xl = cv2_shim.border_interpolate(xs - 1, w, cv2_shim.BORDER_REFLECT_101)
    xr = cv2_shim.border_interpolate(xs + 1, w, cv2_shim.BORDER_REFLECT_101)
    yu = cv2_shim.border_interpolate(ys - 1, h, cv2_shim.BORDER_REFLECT_101)
    yd = cv2_shim.border_interpolate(ys + 1, h, cv2_shim.BORDER_REFLECT_101)
    lap = ((g[:, xl] + g[:, xr]) + (g[yu] + g[yd])) - ft(4) * g
    C = np.abs(lap)
    m = ((B + G) + R) / ft(3)
    S = np.sqrt((((B - m) * (B - m) + (G - m) * (G - m)) + (R - m) * (R - m)) / ft(3))
    half = ft(0.5)
    E = np.exp(-((((B - half) * (B - half) + (G - half) * (G - half)) + (R - half) * (R - half))
                 / ft(np.float32(0.08))))
    prod = np.ones((h, w), ft)
    for factor, e in zip((C, S, E), params):
        f = _power(factor, e, ft)
        if f is not None:
            prod = prod * f
    return (prod + ft(np.float32(1e-12))).astype(ft)


def fuse_from_raw(frames, raws, n_levels=None):
    """Stages B .. E: ``frames`` K uint8 [h][w][3], ``raws`` K float32 [h][w] (stage A's W).
    Returns (fused float32 [h][w][3] before quantisation, uint8 [h][w][3])."""
    f32 = np.float32
    frames = [np.asarray(f) for f in frames]
    raws = [np.asarray(r, f32) for r in raws]
    h, w = frames[0].shape[:2]
    L = levels_for(h, w) if n_levels is None else int(n_levels)
    assert 0 <= L <= levels_for(h, w)
    total = raws[0]
    for r in raws[1:]:
        total = total + r
    pyramids = []
    for frame, r in zip(frames, raws):
        packed = np.empty((h, w, 4), f32)
        packed[..., :3] = frame.astype(f32) / f32(255.0)
        packed[..., 3] = r / total
        pyr = [packed]
        for _ in range(L):
            pyr.append(cv2_shim.pyrDown(pyr[-1]))
        pyramids.append(pyr)
    levels = []
    for l in range(L + 1):
        acc = None
        for pyr in pyramids:
            P = pyr[l]
            d = P[..., :3]
            if l < L:
                d = d - cv2_shim.pyrUp(np.ascontiguousarray(pyr[l + 1][..., :3]))[:P.shape[0], :P.shape[1]]
            term = P[..., 3:4] * d
            acc = term if acc is None else acc + term
        levels.append(acc.astype(f32))
    out = levels[L]
    for l in range(L - 1, -1, -1):
        out = levels[l] + cv2_shim.pyrUp(out)[:levels[l].shape[0], :levels[l].shape[1]]
    assert out.dtype == f32
    q = np.rint(np.minimum(np.maximum(out * f32(255.0), f32(0.0)), f32(255.0))).astype(np.uint8)
    return out, q


def fuse(frames, params=(1.0, 1.0, 1.0), n_levels=None):
    """The whole contract in NumPy's float32: (fused float32, uint8)."""
    return fuse_from_raw(frames, [raw_weights(f, np.float32, params) for f in frames], n_levels)
