"""The contract of ``pano_overlap_stats`` (include/pano360.h, csrc/gains.hip) in NumPy, vectorised
over the frame: every pixel (x, y) of frame i is looked up in frame j as
``cv2.warpPerspective(img_j, hom, (w, h), INTER_LINEAR, BORDER_TRANSPARENT)`` looks it up in the
float32 RGBA image, and counts where the sampled alpha is non-zero.

Per pixel, in float64 with one rounding per operation, x = xb + x1 with xb = (x // bw0) * bw0:

    den = ((m6*xb + m7*y) + m8) + m6*x1          W = 32 / den, or 0 where den == 0
    fX  = (((m0*xb + m1*y) + m2) + m0*x1) * W    fY likewise with m3, m4, m5
    X   = cvRound(fmax(-2^31, fmin(2^31 - 1, fX)))           (ties to even)
    tap = X >> 5 saturated to int16, fraction = X & 31

A pixel is sampled only where all four taps lie inside frame j, ``0 <= sx < w - 1`` and
``0 <= sy < h - 1``; the four weights and both bilinear sums (alpha, colour) are float32, left to
right; alpha per tap is ``float32(hat_y * hat_x)``, a colour is ``float32(u8) / float32(255)``.

Nothing here is shared with the implementations under test (the kernel, the C oracle,
oracle/cv2_shim.py): no import of ``oracle/`` or ``pano360_amd``.  Two switches exist only so
that tests/test_overlap_host.py can show that a case is sharp: ``rounding="away"`` rounds halves
away from zero, and ``split=False`` computes the numerators with xb = x, x1 = 0.
"""
import math
from collections import namedtuple

import numpy as np

# mask: bool [h][w], the counted pixels;  count: their number;  sum_i, sum_j: the correctly rounded
# double sums of frame i's colours and of the sampled colours of frame j over those pixels and the
# three channels;  samples: float32 [count][3], the sampled colours in row-major pixel order
Stats = namedtuple("Stats", "mask count sum_i sum_j samples")

F32 = np.float32
LUT255 = np.arange(256, dtype=F32) / F32(255)
INT32_LO, INT32_HI = -2147483648.0, 2147483647.0


def _round(val, rounding):
    if rounding == "even":
        return np.rint(val).astype(np.int64)
    if rounding != "away":
        raise ValueError(rounding)
    whole = np.trunc(val)
    # val - whole is exact; |val| <= 2^31, so whole +- 1 is exact too
    return (whole + np.where(np.abs(val - whole) >= 0.5, np.sign(val), 0.0)).astype(np.int64)


def denominators(minv, h, w, bw0, split=True):
    """float64 [h][w]: den of every pixel."""
    return _numerators(minv, h, w, bw0, split)[2]


def _numerators(minv, h, w, bw0, split):
    m = np.asarray(minv, np.float64).ravel()
    assert m.size == 9 and h > 0 and w > 0 and bw0 > 0
    col = np.arange(w, dtype=np.int64)
    if split:
        xb = ((col // bw0) * bw0).astype(np.float64)[None, :]
        x1 = (col % bw0).astype(np.float64)[None, :]
    else:
        xb = col.astype(np.float64)[None, :]
        x1 = np.zeros((1, w))
    y = np.arange(h, dtype=np.float64)[:, None]
    return tuple(((m[k] * xb + m[k + 1] * y) + m[k + 2]) + m[k] * x1 for k in (0, 3, 6))


def fixed_point(minv, h, w, bw0, rounding="even", split=True):
    """(X, Y), int64 [h][w]: the source coordinates of every pixel in 1/32 px."""
    num_x, num_y, den = _numerators(minv, h, w, bw0, split)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        scale = np.where(den != 0.0, 32.0 / den, 0.0)
        out = []
        for num in (num_x, num_y):
            # fmin / fmax return the other operand for a NaN, as C's do: 0 * inf ends at 2^31 - 1
            val = np.fmax(INT32_LO, np.fmin(INT32_HI, num * scale))
            out.append(_round(val, rounding))
    return tuple(out)


def taps(minv, h, w, bw0, rounding="even", split=True):
    """(sx, sy, fx, fy, inside): the int16-saturated integer parts, the fractions 0 .. 31, and
    where all four taps lie inside an h x w frame."""
    big_x, big_y = fixed_point(minv, h, w, bw0, rounding, split)
    sx = np.clip(big_x >> 5, -32768, 32767)
    sy = np.clip(big_y >> 5, -32768, 32767)
    inside = (sx >= 0) & (sx < w - 1) & (sy >= 0) & (sy < h - 1)
    return sx, sy, big_x & 31, big_y & 31, inside


def _lerp4(v00, v01, v10, v11, wgt):
    acc = v00 * wgt[0]
    acc = acc + v01 * wgt[1]
    acc = acc + v10 * wgt[2]
    acc = acc + v11 * wgt[3]
    assert acc.dtype == F32
    return acc


def overlap(frame_i, frame_j, minv, bw0, hat_x, hat_y, rounding="even", split=True):
    """The ``Stats`` of one pair.  frame_i, frame_j: uint8 [h][w][3]; minv: 9 doubles;
    hat_x [w], hat_y [h]: float64."""
    frame_i, frame_j = np.asarray(frame_i), np.asarray(frame_j)
    h, w = frame_i.shape[:2]
    assert frame_i.dtype == frame_j.dtype == np.uint8 and frame_i.shape == frame_j.shape == (h, w, 3)
    hat_x, hat_y = np.asarray(hat_x, np.float64), np.asarray(hat_y, np.float64)
    assert hat_x.shape == (w,) and hat_y.shape == (h,)
    sx, sy, fx, fy, inside = taps(minv, h, w, bw0, rounding, split)
    py, px = np.nonzero(inside)                              # row-major
    x0, y0 = sx[py, px], sy[py, px]
    one = F32(1.0)
    ax = fx[py, px].astype(F32) * F32(1.0 / 32.0)
    ay = fy[py, px].astype(F32) * F32(1.0 / 32.0)
    wgt = ((one - ay) * (one - ax), (one - ay) * ax, ay * (one - ax), ay * ax)
    alpha = (hat_y[:, None] * hat_x[None, :]).astype(F32)
    sampled_alpha = _lerp4(alpha[y0, x0], alpha[y0, x0 + 1], alpha[y0 + 1, x0],
                           alpha[y0 + 1, x0 + 1], wgt)
    keep = sampled_alpha != 0
    py, px, x0, y0 = py[keep], px[keep], x0[keep], y0[keep]
    wgt = tuple(v[keep][:, None] for v in wgt)
    colour = LUT255[frame_j]
    samples = _lerp4(colour[y0, x0], colour[y0, x0 + 1], colour[y0 + 1, x0],
                     colour[y0 + 1, x0 + 1], wgt)
    mask = np.zeros((h, w), bool)
    mask[py, px] = True
    own = LUT255[frame_i][py, px]
    return Stats(mask, int(len(py)), math.fsum(own.astype(np.float64).ravel()),
                 math.fsum(samples.astype(np.float64).ravel()), samples)
