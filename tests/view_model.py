"""NumPy float64 model of the view stage (``pano_mip_u8``, ``pano_view_render`` of
include/pano360.h; csrc/view.hip): the record of its semantics.

A mosaic of H x W pixels samples the sphere at theta = low[0] + x res[0], phi = low[1] + y res[1]
(frame: x right, y down, z forward; theta = atan2(x, z), phi = atan2(y, hypot(x, z))).  ``geom`` is
anything with ``low``, ``resolution``, ``shape`` and ``closed`` (``view.MosaicGeometry``); ``view`` is
anything with ``kind``, ``w``, ``h``, ``mat`` (3 x 3) and ``params`` (4 values) (``view.View``).

The device computes in float32; it is compared with this model within one grey level, away from
the pixels ``near_boundary`` marks (tests/test_gpu_view.py)."""
import numpy as np

RECTILINEAR, EQUIRECT, STEREOGRAPHIC = 0, 1, 2
MAX_LEVELS = 16
TWO_PI = 2.0 * np.pi


def mip_levels(img):
    """The levels of a uint8 [H][W][3] image: level l + 1 is ((H_l + 1) // 2, (W_l + 1) // 2), a
    pixel (a + b + c + d + 2) >> 2 over its 2 x 2 block, the odd index clamped to the last row or
    column; they stop at 1 x 1 or at MAX_LEVELS levels."""
    levels = [np.ascontiguousarray(img, np.uint8)]
    while len(levels) < MAX_LEVELS and levels[-1].shape[:2] != (1, 1):
        src = levels[-1].astype(np.int32)
        h, w = src.shape[:2]
        ys, xs = np.arange((h + 1) // 2) * 2, np.arange((w + 1) // 2) * 2
        y1, x1 = np.minimum(ys + 1, h - 1), np.minimum(xs + 1, w - 1)
        total = (src[ys][:, xs] + src[ys][:, x1] + src[y1][:, xs] + src[y1][:, x1] + 2) >> 2
        levels.append(total.astype(np.uint8))
    return levels


def directions(view, u, v):
    """Direction d [..][3] of the output pixels (u, v) (arrays that broadcast)."""
    u, v = np.broadcast_arrays(np.asarray(u, np.float64), np.asarray(v, np.float64))
    mat = np.asarray(view.mat, np.float64)
    p = [float(x) for x in view.params]
    if view.kind == RECTILINEAR:
        cam = np.stack([u, v, np.ones_like(u)], axis=-1)
    elif view.kind == EQUIRECT:
        th, ph = p[0] + u * p[1], p[2] + v * p[3]
        cam = np.stack([np.cos(ph) * np.sin(th), np.sin(ph), np.cos(ph) * np.cos(th)], axis=-1)
    elif view.kind == STEREOGRAPHIC:
        x, y = (u - p[0]) / p[2], (v - p[1]) / p[2]
        cam = np.stack([4 * x, 4 * y, 4 - (x * x + y * y)], axis=-1)
    else:
        raise ValueError(view.kind)
    return cam @ mat.T


def angles(view, u, v):
    d = directions(view, u, v)
    theta = np.arctan2(d[..., 0], d[..., 2])
    phi = np.arctan2(d[..., 1], np.hypot(d[..., 0], d[..., 2]))
    return theta, phi


def _column_scale(geom):
    """fx is brought into [0, period); on a closed mosaic it is stretched so the period is W."""
    period = TWO_PI / float(geom.resolution[0])
    return period, (geom.shape[1] / period if geom.closed else 1.0)


def coordinates(view, geom):
    """(fx, fy, covered, lod) of every output pixel, each [h][w]."""
    H, W = geom.shape
    low, res = np.asarray(geom.low, np.float64), np.asarray(geom.resolution, np.float64)
    v, u = np.meshgrid(np.arange(view.h), np.arange(view.w), indexing="ij")
    theta, phi = angles(view, u, v)
    period, scale = _column_scale(geom)
    fx = np.mod((theta - low[0]) / res[0], period)
    fx = np.where(fx >= period, fx - period, fx) * scale
    fy = (phi - low[1]) / res[1]
    covered = (fy >= 0) & (fy <= H - 1)
    if not geom.closed:
        covered &= fx <= W - 1
    rho = np.zeros(theta.shape)
    for du, dv in ((1, 0), (0, 1)):
        t1, p1 = angles(view, u + du, v + dv)
        dth = t1 - theta
        dth = dth - TWO_PI * np.ceil((dth - np.pi) / TWO_PI)          # into (-pi, pi]
        rho = np.maximum(rho, np.hypot(dth / res[0] * scale, (p1 - phi) / res[1]))
    with np.errstate(divide="ignore"):
        lod = np.log2(rho)
    return fx, fy, covered, lod


def near_boundary(view, geom, eps=1e-3):
    """Pixels whose fx or fy lies within ``eps`` px of a coverage boundary: fy = 0 and H - 1, and
    on an open mosaic fx = W - 1 and the wrap point fx = 0 = period.  Rounding may flip their
    coverage: comparisons with the device leave them out."""
    H, W = geom.shape
    fx, fy, _, _ = coordinates(view, geom)
    near = (np.abs(fy) <= eps) | (np.abs(fy - (H - 1)) <= eps)
    if not geom.closed:
        period, _ = _column_scale(geom)
        near |= (np.abs(fx - (W - 1)) <= eps) | (fx <= eps) | (period - fx <= eps)
    return near


def _bilinear(level, fx, fy, shift, closed):
    """Bilinear sample of one level at the level coordinate (f - (2^l - 1) / 2) / 2^l: rows
    clamped, columns clamped (open) or taken modulo the level's width (closed)."""
    h, w = level.shape[:2]
    size = float(1 << shift)
    cx, cy = (fx - (size - 1) / 2) / size, (fy - (size - 1) / 2) / size
    x0, y0 = np.floor(cx), np.floor(cy)
    ax, ay = (cx - x0)[..., None], (cy - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    fold = (lambda x: np.mod(x, w)) if closed else (lambda x: np.clip(x, 0, w - 1))
    xa, xb = fold(x0), fold(x0 + 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    lv = level.astype(np.float64)
    top = lv[ya, xa] + ax * (lv[ya, xb] - lv[ya, xa])
    bot = lv[yb, xa] + ax * (lv[yb, xb] - lv[yb, xa])
    return top + ay * (bot - top)


def render(levels, geom, view):
    """(image uint8 [h][w][3], mask uint8 [h][w]) of one view: trilinear between the levels
    floor(lod) and floor(lod) + 1, lod = clamp(log2 rho, 0, L - 1); floor(x + 0.5) clamped to
    0 .. 255; uncovered pixels 0 in both."""
    fx, fy, covered, lod = coordinates(view, geom)
    n = len(levels)
    lod = np.clip(np.where(np.isnan(lod), 0.0, lod), 0.0, n - 1.0)
    l0 = np.minimum(np.floor(lod).astype(np.int64), n - 1)
    t = (lod - l0)[..., None]
    out = np.zeros(fx.shape + (3,))
    for level in range(n):
        for which in (0, 1):                        # as the lower, as the upper level of a pixel
            sel = (l0 == level - which) & (True if which == 0 else (lod - l0 > 0))
            if not sel.any():
                continue
            val = _bilinear(levels[level], fx[sel], fy[sel], level, geom.closed)
            out[sel] += val * (t[sel] if which else 1.0 - t[sel])
    img = np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)
    img[~covered] = 0
    return img, covered.astype(np.uint8)


def levels_crossed(view, geom, n_levels):
    """The set of floor(lod) values over the covered pixels of a view."""
    _, _, covered, lod = coordinates(view, geom)
    lod = np.clip(np.where(np.isnan(lod), 0.0, lod), 0.0, n_levels - 1.0)
    return set(np.floor(lod[covered]).astype(int).tolist())
