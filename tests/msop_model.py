"""The MSOP detector's arithmetic in NumPy: the specification of csrc/msop.hip.

What the reference's ``msop_detect`` / ``ssc`` / ``_msop_descriptors`` (features.py:27-156) get
from OpenCV is restated from OpenCV's published behaviour (PARITY UNPINNED: OpenCV is not in the
reference repo), float32 with one rounding per operation and float64 where OpenCV uses double:

* ``gray_u8``      cvtColor(BGR2GRAY) on 8-bit: (B 1868 + G 9617 + R 4899 + 2^13) >> 14.
* ``sobel``        Sobel 3 x 3, REFLECT_101, row pass then column pass: the difference is
                   ``p[+1] - p[-1]``, the smoothing ``(p[-1] + p[+1]) + 2 p[0]``.
* ``corner_harris`` cornerHarris(blockSize 2, ksize 3, k): Sobel scaled by 1/8, the three product
                   planes, the unnormalised 2 x 2 box sum with anchor (1, 1) and REFLECT_101
                   ``(p[y-1][x-1] + p[y-1][x]) + (p[y][x-1] + p[y][x])``, then
                   ``a c - b b - k (a + c) (a + c)`` left to right.
* ``warp_perspective`` warpPerspective(INTER_LINEAR, BORDER_CONSTANT 0) for any matrix (what
                   the golden generator hands the reference), ``patch`` the closed form of the
                   map the reference builds (the contract of the kernel).
* ``normalise``    ``(t - mean) / (std + 1e-8)`` with NumPy's pairwise float32 sum of 64 values.

The Gaussian filters and pyrDown are the oracle's stand-ins (oracle/cv2_shim.py), the ones
``pano_blur_plane`` and ``pano_pyr_down`` are already tested against.

Kept quirks of the reference: the cut hands its points on weakest first; ``ssc`` names
``cols, rows = (H, W)`` and reads ``kpt[0]`` (the row) as x; ``theta = arctan2(g_x, g_y)``;
``KeyPoint.size`` carries theta.  This project's own rule: equal responses at the cut are ordered
by ascending row-major position (a stable argsort; NumPy's default leaves the order open), and
-0.0 equals +0.0.
"""
import math

import numpy as np

import cv2_shim

DSIZE = 8
HARRIS_K = 0.04
f32 = np.float32


def gray_u8(img):
    """float32(cvtColor(img, BGR2GRAY)) of a uint8 [h][w][3] image."""
    p = np.asarray(img, np.uint8).astype(np.int64)
    return ((p[..., 0] * 1868 + p[..., 1] * 9617 + p[..., 2] * 4899 + (1 << 13)) >> 14).astype(f32)


def _pad101(p, n=1):
    h, w = p.shape
    ry = cv2_shim.border_interpolate(np.arange(-n, h + n), h, cv2_shim.BORDER_REFLECT_101)
    rx = cv2_shim.border_interpolate(np.arange(-n, w + n), w, cv2_shim.BORDER_REFLECT_101)
    return p[ry][:, rx]


def sobel(gray, dx, dy, scale=1.0):
    """cv2.Sobel(gray, CV_32F, dx, dy, ksize=3, scale) for (dx, dy) = (1, 0) or (0, 1)."""
    g = _pad101(np.asarray(gray, f32))
    if (dx, dy) == (1, 0):
        row = g[:, 2:] - g[:, :-2]
        out = (row[:-2] + row[2:]) + row[1:-1] * f32(2)
    elif (dx, dy) == (0, 1):
        row = (g[:, :-2] + g[:, 2:]) + g[:, 1:-1] * f32(2)
        out = row[2:] - row[:-2]
    else:
        raise NotImplementedError((dx, dy))
    return (out * f32(scale)).astype(f32)


def corner_harris(gray, k=HARRIS_K):
    """cv2.cornerHarris(gray, blockSize=2, ksize=3, k) on a float32 plane."""
    dx, dy = sobel(gray, 1, 0, 0.125), sobel(gray, 0, 1, 0.125)
    planes = []
    for p in (dx * dx, dx * dy, dy * dy):
        q = _pad101(p)[:-1, :-1]                    # rows y-1 .. y, columns x-1 .. x
        planes.append((q[:-1, :-1] + q[:-1, 1:]) + (q[1:, :-1] + q[1:, 1:]))
    a, b, c = planes
    return (a * c - b * b - f32(k) * (a + c) * (a + c)).astype(f32)


def candidates(hrs):
    """Row-major flat positions of the pixels that are >= all 8 neighbours (a 3 x 3 maximum
    filter with SciPy's ``reflect`` border: what lies outside repeats the edge)."""
    h, w = hrs.shape
    p = np.pad(hrs, 1, mode="symmetric")
    best = hrs.copy()
    for oy in range(3):
        for ox in range(3):
            best = np.maximum(best, p[oy:oy + h, ox:ox + w])
    return np.flatnonzero((best == hrs).reshape(-1))


def cut(hrs, maxf):
    """The last 20 maxf candidates in ascending order of response, ties by ascending position:
    int64 [n][2] (row, col), weakest first."""
    pos = candidates(hrs)
    order = np.argsort(hrs.reshape(-1)[pos] + f32(0), kind="stable")[-20 * maxf:]
    pos = pos[order]
    return np.stack([pos // hrs.shape[1], pos % hrs.shape[1]], axis=1)


def search_ceiling(rows, cols, n_points):
    """The upper end of ``ssc``'s search range (features.py:40-61): the larger root, negated and
    rounded half to even, of the suppression-square quadratic of Bailo et al.  Written with half
    the linear coefficient, ``w = -(half_b +- sqrt(quarter_disc)) / (n_points - 1)``; the integer
    arithmetic is exact, float64 starts at the square root."""
    half_b = rows + cols + 2 * n_points
    quarter_disc = (rows - cols) ** 2 + 4 * (cols + n_points * (1 + rows + rows * cols))
    root = math.sqrt(quarter_disc)
    return max(-round((half_b + sign * root) / (n_points - 1)) for sign in (1, -1))


class SscSearch:
    """The scalar control of ``ssc``'s binary search (features.py:36-61, 64-69, 91-97) in Python
    float64 and Python ``round``: ``next_width()`` gives the width to probe or None when the
    search is over, ``report(count)`` takes the probe's count.  ``im_size`` = (H, W) is read as
    (cols, rows), the reference's swap."""

    def __init__(self, n_keypoints, im_size, n_points, tol=0.1):
        if n_points == 1:
            raise ValueError("ssc: n_points = 1 divides by zero in the search range")
        self.cols, self.rows = im_size
        self.high = search_ceiling(self.rows, self.cols, n_points)
        self.low = math.floor(math.sqrt(n_keypoints / n_points))
        self.k_min = round(n_points - n_points * tol)
        self.k_max = round(n_points + n_points * tol)
        self.prev_width, self.complete, self.width = -1, False, None

    def next_width(self):
        if self.complete:
            return None
        width = self.low + (self.high - self.low) / 2
        if width == self.prev_width or self.low > self.high:
            return None
        self.width = width
        return width

    def grid(self):
        """(cgr, cell rows - 1, cell columns - 1, reach) of the width to probe."""
        cgr = self.width / 2
        return (cgr, int(math.floor(self.rows / cgr)), int(math.floor(self.cols / cgr)),
                int(math.floor(self.width / cgr)))

    def report(self, count):
        if self.k_min <= count <= self.k_max:
            self.complete = True
        elif count < self.k_min:
            self.high = self.width - 1
        else:
            self.low = self.width + 1
        self.prev_width = self.width


def ssc_probe(points, cgr, n_cell_rows, n_cell_cols, reach):
    """One greedy walk: a point is taken if its cell (floor(kpt[1] / cgr), floor(kpt[0] / cgr))
    is uncovered, and covers the cells within ``reach`` of its own, clipped to the grid."""
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    rows = np.floor(pts[:, 1] / cgr).astype(np.int64).tolist()
    cols = np.floor(pts[:, 0] / cgr).astype(np.int64).tolist()
    stride = n_cell_cols + 1
    buf = bytearray((n_cell_rows + 1) * stride)
    cov = np.frombuffer(buf, np.uint8).reshape(n_cell_rows + 1, stride)
    result = []
    for i, (row, col) in enumerate(zip(rows, cols)):
        if not buf[row * stride + col]:
            result.append(i)
            cov[max(row - reach, 0):min(row + reach, n_cell_rows) + 1,
                max(col - reach, 0):min(col + reach, n_cell_cols) + 1] = 1
    return result


def ssc_indices(points, im_size, n_points, tol=0.1):
    """Indices ``ssc`` selects, in walk order: those of the last probe that ran."""
    search = SscSearch(len(points), im_size, n_points, tol)
    result = []
    while search.next_width() is not None:
        result = ssc_probe(points, *search.grid())
        search.report(len(result))
    return result


def ssc(keypoints, im_size, n_points, tol=0.1):
    return [keypoints[i] for i in ssc_indices(keypoints, im_size, n_points, tol)]


def gradient_planes(gray):
    """(g_x, g_y, blurred) of ``_msop_descriptors`` (features.py:112-114)."""
    blur = lambda p, sigma: cv2_shim.GaussianBlur(p, (gaussian_ksize(sigma),) * 2, sigma, sigma)  # noqa: E731
    return blur(sobel(gray, 1, 0), 1.0), blur(sobel(gray, 0, 1), 1.0), blur(gray, 2.0)


def gaussian_ksize(sigma):
    """features.py:22-23."""
    ksz = max(int((sigma - 0.35) / 0.15), 1)
    return ksz + (not ksz % 2)


def thetas(g_x, g_y, rows, cols):
    return np.arctan2(g_x[rows, cols], g_y[rows, cols]).astype(f32)


def _sample(src, big_x, big_y):
    """OpenCV's fixed-point bilinear tap sum at X = 32 x, Y = 32 y (integers), constant border 0."""
    h, w = src.shape
    sx, sy = big_x >> 5, big_y >> 5
    ax = (big_x & 31).astype(f32) * f32(1.0 / 32)
    ay = (big_y & 31).astype(f32) * f32(1.0 / 32)
    one = f32(1)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(ok, src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], f32(0))

    acc = tap(sy, sx) * ((one - ay) * (one - ax))
    acc = acc + tap(sy, sx + 1) * ((one - ay) * ax)
    acc = acc + tap(sy + 1, sx) * (ay * (one - ax))
    acc = acc + tap(sy + 1, sx + 1) * (ay * ax)
    return acc.astype(f32)


def warp_perspective(src, M, dsize, flags=cv2_shim.INTER_LINEAR,
                     borderMode=cv2_shim.BORDER_CONSTANT):
    """cv2.warpPerspective of a float32 plane for any 3 x 3 ``M`` (src -> dst): ``M`` inverted in
    double (cv::invert: adjugate / det), the coordinates per destination pixel in double
    (``X0 = M1 y + M2``, ``W = 32 / (M7 y + M8 + M6 x)``, ``X = rint((X0 + M0 x) W)``)."""
    if flags != cv2_shim.INTER_LINEAR or borderMode != cv2_shim.BORDER_CONSTANT:
        raise NotImplementedError((flags, borderMode))
    width, height = dsize
    assert width <= cv2_shim.warp_block_width(width, height)      # one column block: x1 = x
    m = cv2_shim.invert3x3(np.asarray(M, np.float64)).ravel()
    x = np.arange(width, dtype=np.float64)[None, :]
    y = np.arange(height, dtype=np.float64)[:, None]
    x0 = m[0] * 0.0 + m[1] * y + m[2]
    y0 = m[3] * 0.0 + m[4] * y + m[5]
    w0 = m[6] * 0.0 + m[7] * y + m[8]
    den = w0 + m[6] * x
    with np.errstate(divide="ignore", invalid="ignore"):
        wgt = np.where(den != 0.0, 32.0 / den, 0.0)
    big_x = np.rint((x0 + m[0] * x) * wgt).astype(np.int64)
    big_y = np.rint((y0 + m[3] * x) * wgt).astype(np.int64)
    return _sample(np.ascontiguousarray(src, f32), big_x, big_y)


def patches(blurred, theta, rows, cols):
    """The raw 8 x 8 tiles [n][8][8] around (rows, cols), turned by float32 ``theta``: the closed
    form of the reference's map (features.py:120-123), in double:
    x_src = cs (u - 4) + sn (v - 4) + c, y_src = -sn (u - 4) + cs (v - 4) + r with
    cs = float32(cos(double(theta))), sn likewise."""
    th = np.asarray(theta, f32).astype(np.float64)
    cs = np.cos(th).astype(f32).astype(np.float64)[:, None, None]
    sn = np.sin(th).astype(f32).astype(np.float64)[:, None, None]
    u = (np.arange(DSIZE, dtype=np.float64) - DSIZE / 2)[None, None, :]
    v = (np.arange(DSIZE, dtype=np.float64) - DSIZE / 2)[None, :, None]
    c = np.asarray(cols, np.float64)[:, None, None]
    r = np.asarray(rows, np.float64)[:, None, None]
    x_src = cs * u + sn * v + c
    y_src = -sn * u + cs * v + r
    big_x = np.rint(32.0 * x_src).astype(np.int64)
    big_y = np.rint(32.0 * y_src).astype(np.int64)
    return _sample(np.ascontiguousarray(blurred, f32), big_x, big_y)


def _sum64(t):
    """NumPy's pairwise sum of 64 contiguous float32: 8 strided accumulators."""
    t = np.asarray(t, f32).reshape(-1, 8, 8)
    r = t[:, 0, :].copy()
    for i in range(1, 8):
        r = r + t[:, i, :]
    return ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))


def normalise(tiles):
    """(t - mean(t)) / (std(t) + 1e-8) of [n][64] float32, as NumPy evaluates it."""
    t = np.asarray(tiles, f32).reshape(-1, 64)
    mean = (_sum64(t) / f32(64))[:, None]
    dev = t - mean
    std = np.sqrt(_sum64(dev * dev) / f32(64))[:, None]
    return ((t - mean) / (std + f32(1e-8))).astype(f32)


def rot_mat(theta, pp_):
    """features.py:102-106: turn by ``theta``, then move the origin to ``pp_`` = (row, col);
    float32, rows in (x, y, 1) order."""
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([f32([c, s, pp_[1]]), f32([-s, c, pp_[0]]), f32([0, 0, 1])])


def detect_level(gray, maxf, scale, theta=None):
    """One level of ``msop_detect`` on a float32 plane: a dict of every stage.  ``theta``
    (float32 [n]) replaces the model's own angles (the GPU test hands in the device's)."""
    hrs = corner_harris(gray)
    cut_rc = cut(hrs, maxf)
    sel = ssc_indices(cut_rc, gray.shape, maxf)
    if not sel:
        raise ValueError("msop_detect: ssc left a level without points")
    rows, cols = cut_rc[sel, 0], cut_rc[sel, 1]
    g_x, g_y, blurred = gradient_planes(gray)
    th = thetas(g_x, g_y, rows, cols) if theta is None else np.asarray(theta, f32)
    tiles = patches(blurred, th, rows, cols)
    points = np.stack([scale * rows.astype(np.float64), scale * cols.astype(np.float64),
                       th.astype(np.float64), np.full(len(rows), float(scale))], axis=1)
    return {"hrs": hrs, "cut": cut_rc, "sel": np.asarray(sel, np.int64), "g_x": g_x, "g_y": g_y,
            "blurred": blurred, "theta": th, "tiles": tiles, "desc": normalise(tiles),
            "points": points}


def detect(img, max_feat=(5000, 100, 25, 10), thetas_in=None, want_stages=False):
    """``msop_detect`` (features.py:133-156): (points float64 [N][4], descs float32 [N][64])."""
    gray = gray_u8(img)
    stages = []
    for lvl, maxf in enumerate(max_feat):
        stages.append(detect_level(gray, maxf, 2 ** lvl,
                                   None if thetas_in is None else thetas_in[lvl]))
        gray = cv2_shim.pyrDown(gray)
    out = (np.concatenate([s["points"] for s in stages]),
           np.concatenate([s["desc"] for s in stages]))
    return out + (stages,) if want_stages else out


class KeyPoint:
    """The fields of ``cv2.KeyPoint`` the reference sets (features.py:208)."""

    def __init__(self, x, y, size):
        self.pt, self.size = (float(x), float(y)), float(size)


# ---------------------------------------------------------------- the test inputs
def smooth_noise(h, w, seed, sigma=2.0):
    """A Gaussian-smoothed random uint8 plane, stretched to the full range."""
    rng = np.random.default_rng(seed)
    p = cv2_shim.GaussianBlur(rng.random((h, w)).astype(f32), (0, 0), sigma)
    p = (p - p.min()) / (p.max() - p.min())
    return np.rint(p * 255).astype(np.uint8)


def fixture_image(name):
    """The uint8 BGR inputs of the golden cases (tools/gen_msop_golden.py)."""
    if name == "noise":
        return np.repeat(smooth_noise(192, 256, 7)[..., None], 3, axis=2)
    if name == "odd":
        return np.stack([smooth_noise(157, 203, 11 + c) for c in range(3)], axis=2)
    if name == "flat":
        img = np.repeat(smooth_noise(192, 256, 13)[..., None], 3, axis=2)
        img[20:60, 30:90] = 255
        img[100:150, 140:220] = 0
        img[150:180, 10:50] = 255
        return img
    raise KeyError(name)


def shifted_pair():
    """Two 192 x 256 crops of one 240 x 400 texture, offset by (dy, dx) = (16, 72)."""
    tex = np.repeat(smooth_noise(240, 400, 21)[..., None], 3, axis=2)
    return tex[0:192, 0:256].copy(), tex[16:208, 72:328].copy()
