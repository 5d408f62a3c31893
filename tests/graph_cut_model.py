"""NumPy restatement of the reference's ``blend.graph_cut`` and ``blend.alpha_blend``
(blend.py:48-100), written from their observed behaviour and pinned to the reference by the label
grids and masks stored in tests/golden/graph_cut_*.npz (tools/gen_graph_cut_golden.py).

``graph_cut`` is a two-marker priority flood on a grid of *levels*:

``levels``       the per-pixel difference ``max over channels |img1 - img2|`` (-1 where a fourth
                 channel is 0 in either image), cropped to a multiple of ``shrink`` and reduced by
                 the minimum over ``shrink x shrink`` cells.  The level of a cell is the priority
                 the flood gives it, higher first.  For signed integer and float images holding
                 the integers 0..255 it is the difference itself (-1 .. 255).  uint8 images make
                 the reference subtract *and negate* in uint8: its difference wraps
                 (``3 - 5 = 254``) and so does the heap key ``-diff`` (``-0 = 0``, ``-d = 256 - d``),
                 which puts a difference of 0 first and then 255, 254, .. 1.  That order is
                 restated as ``level = 255 where diff == 0, else diff - 1``.
``flood_heap``   the reference's loop, literally: a heap of ``(-level, colour, x, y)``.
``flood_sweep``  the same labels without a heap.  The labels depend only on the order of the
                 classes ``(level descending, colour -1 before +1)``: while ``(d, c)`` is the
                 smallest class on the heap every entry the flood creates has colour ``c``, and
                 those of a level ``>= d`` sort before everything of the other colour still
                 waiting.  So a class labels with ``c`` every connected component of unlabelled
                 cells of level ``>= d`` that touches a ``c``-labelled cell, and afterwards every
                 entry left belongs to a later class.
``mask_from_labels``  ``cv2.resize`` (bilinear, float32) of ``labels == -1`` to the image size,
                 times 255, truncated to uint8: OpenCV's float path restated (parity unpinned, as
                 for every OpenCV call the reference makes).
"""
import heapq

import numpy as np

DTYPES = (np.uint8, np.int16, np.int32, np.float32, np.float64)


def border_of(shrink):
    """Width of the two preset bands (blend.py:74)."""
    return int(13 / shrink) + 1


def levels(img1, img2, shrink=5):
    """int16 ``[H // shrink][W // shrink]`` grid of flood priorities (module docstring)."""
    img1, img2 = np.asarray(img1), np.asarray(img2)
    wrapped = img1.dtype == np.uint8
    if wrapped:
        diff = ((img1.astype(np.int32) - img2.astype(np.int32)) & 255).max(axis=2)
    else:
        diff = np.abs(img1.astype(np.float64) - img2.astype(np.float64)).max(axis=2)
        assert np.array_equal(diff, np.rint(diff)) and diff.min() >= 0 and diff.max() <= 255
        diff = diff.astype(np.int32)
    if img1.shape[2] == 4:
        if wrapped:
            raise OverflowError("the reference cannot store -1 in its uint8 differences")
        diff[img1[:, :, 3] == 0] = -1
        diff[img2[:, :, 3] == 0] = -1
    if shrink > 1:
        rows, cols = diff.shape[0] // shrink, diff.shape[1] // shrink
        diff = diff[:shrink * rows, :shrink * cols]
        diff = diff.reshape(rows, shrink, cols, shrink).min(axis=(1, 3))
    if wrapped:
        diff = np.where(diff == 0, 255, diff - 1)
    return diff.astype(np.int16)


def presets(rows, cols, border):
    """Labels before the flood (blend.py:71-76) and after the seeds of both colours have been
    popped: they all carry the key -1e3, below every cell's, and the -1 seeds sort first."""
    if rows < 1 or cols < 2 * border + 1:
        raise ValueError(f"a {rows} x {cols} grid is too small for bands of {border} columns")
    lab = np.zeros((rows, cols), np.int8)
    lab[:, :border] = -1
    if border == 1:
        lab[:] = 1                          # the reference's slice [:, -0:] is the whole grid
    else:
        lab[:, cols - border + 1:] = 1
    for colour, col in ((-1, border), (1, cols - border)):
        lab[lab[:, col] == 0, col] = colour
    return lab


def flood_heap(level, border):
    """The reference's loop (blend.py:71-97) on a level grid; int8 labels."""
    rows, cols = level.shape
    presets(rows, cols, border)             # the size check
    key = (-level.astype(np.int64)).tolist()
    lab = [[0] * cols for _ in range(rows)]
    for row in lab:
        row[:border] = [-1] * border
        if border > 1:
            row[cols - border + 1:] = [1] * (border - 1)
        else:
            row[:] = [1] * cols
    heap = []
    for y in range(rows):
        heap += [(-1e3, -1, border, y), (-1e3, 1, cols - border, y)]
    heapq.heapify(heap)
    while heap:
        _, colour, x, y = heapq.heappop(heap)
        if lab[y][x] != 0:
            continue
        lab[y][x] = colour
        for dx, dy in ((0, 1), (0, -1), (1, 0), (-1, 0)):
            nx, ny = x + dx, y + dy
            if 0 <= nx < cols and 0 <= ny < rows and lab[ny][nx] == 0:
                heapq.heappush(heap, (key[ny][nx], colour, nx, ny))
    return np.array(lab, np.int8)


def _touching(lab, colour):
    """Cells with a 4-neighbour labelled ``colour``."""
    has = lab == colour
    out = np.zeros_like(has)
    out[1:] |= has[:-1]
    out[:-1] |= has[1:]
    out[:, 1:] |= has[:, :-1]
    out[:, :-1] |= has[:, 1:]
    return out


def flood_sweep(level, border, want_stats=False, stop_below=None):
    """The class sweep (module docstring); with ``want_stats`` also the number of classes that
    labelled at least one cell.  ``stop_below``: leave the levels under it undone (the state of
    the flood part-way, for tests)."""
    from scipy import ndimage
    rows, cols = level.shape
    lab = presets(rows, cols, border)
    worked = 0
    for d in np.unique(level)[::-1]:
        if stop_below is not None and d < stop_below:
            break
        free = (lab == 0) & (level >= d)
        if not free.any():
            continue
        comp, n = ndimage.label(free)       # 4-connected components
        for colour in (-1, 1):
            ids = np.zeros(n + 1, bool)
            ids[comp[_touching(lab, colour) & (lab == 0) & free]] = True
            ids[0] = False
            if ids.any():
                worked += 1
                lab[ids[comp] & (lab == 0)] = colour
    return (lab, worked) if want_stats else lab


def resize_taps(n_out, n_in):
    """Per output sample of ``cv2.resize``'s float bilinear pass: (first tap, second tap) and the
    float32 weights (1 - f, f).  ``scale = 1 / (n_out / n_in)`` in double as OpenCV forms it,
    the source coordinate ``float((d + 0.5) * scale - 0.5)``, floor and fraction, clamped to the
    first / last sample with fraction 0."""
    scale = 1.0 / (float(n_out) / float(n_in))
    f = ((np.arange(n_out) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    f[s < 0] = 0
    s[s < 0] = 0
    f[s >= n_in - 1] = 0
    s[s >= n_in - 1] = n_in - 1
    taps = np.stack([s, np.minimum(s + 1, n_in - 1)], axis=1).astype(np.int32)
    weights = np.stack([np.float32(1.0) - f, f], axis=1).astype(np.float32)
    return taps, weights


def resize_f32(src, dsize):
    """``cv2.resize(src, dsize)`` of a float32 plane, INTER_LINEAR: the horizontal pass
    ``s0*a0 + s1*a1``, then the vertical ``r0*b0 + r1*b1``, float32 with one rounding per
    operation."""
    src = np.ascontiguousarray(src, np.float32)
    width, height = dsize
    xt, xw = resize_taps(width, src.shape[1])
    yt, yw = resize_taps(height, src.shape[0])
    rows = src[:, xt[:, 0]] * xw[None, :, 0] + src[:, xt[:, 1]] * xw[None, :, 1]
    return rows[yt[:, 0]] * yw[:, 0, None] + rows[yt[:, 1]] * yw[:, 1, None]


def mask_from_labels(lab, height, width):
    """blend.py:99-100: uint8 ``[height][width][1]``."""
    mask = resize_f32((lab == -1).astype(np.float32), (width, height))
    return (mask[..., None] * 255).astype(np.uint8)


def graph_cut(img1, img2, shrink=5, flood=flood_sweep):
    """The whole call; returns (labels, mask)."""
    level = levels(img1, img2, shrink)
    border = border_of(shrink)
    if border == 1:
        presets(*level.shape, border)
        lab = np.ones(level.shape, np.int8)
    else:
        lab = flood(level, border)
    return lab, mask_from_labels(lab, img1.shape[0], img1.shape[1])


def default_alpha_mask(width):
    return np.linspace(1, 0, width).reshape((1, width, 1))


def alpha_blend(img1, img2, mask=None):
    """blend.py:48-53 with every step spelled out: the two products and the sum are separate
    roundings in NumPy's promoted type, the result truncated to uint8."""
    if mask is None:
        mask = default_alpha_mask(img1.shape[1])
    mask = np.asarray(mask)
    kind = np.result_type(img1.dtype, mask.dtype)
    rest = (mask.dtype.type(1) - mask).astype(kind)
    first = img1.astype(kind) * mask.astype(kind)
    second = img2.astype(kind) * rest
    return (first + second).astype(np.uint8)


# ---------------------------------------------------------------- seeded inputs
def smooth_pair(height, width, chans, seed, dtype=np.int16, wobble=40.0, noise=0.6):
    """Two smooth images of integers 0..255 that differ by a slowly varying offset plus a little
    noise: a seam with many levels in play."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:height, :width].astype(np.float64)
    out = []
    for k in range(2):
        planes = []
        for c in range(chans):
            ph = rng.uniform(0, 2 * np.pi, 4)
            fr = rng.uniform(0.01, 0.05, 4)
            base = 128 + 50 * np.sin(fr[0] * x + ph[0]) * np.cos(fr[1] * y + ph[1])
            base += k * wobble * np.sin(fr[2] * x + fr[3] * y + ph[2])
            base += rng.normal(0, noise, base.shape)
            planes.append(base)
        out.append(np.clip(np.rint(np.stack(planes, axis=2)), 0, 255).astype(dtype))
    return out


def noise_pair(height, width, chans, seed, dtype=np.int16):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (height, width, chans)).astype(dtype) for _ in range(2)]


def island_pair(height, width, chans, seed, dtype=np.int16):
    """Pockets of high difference walled in by rings of low difference, on a mid-level noisy
    ground: the pockets stay unlabelled while the flood passes them and are taken late."""
    rng = np.random.default_rng(seed)
    one = rng.integers(60, 120, (height, width, chans))
    gap = rng.integers(20, 90, (height, width))
    y, x = np.mgrid[:height, :width]
    for _ in range(14):
        cy, cx = rng.integers(8, height - 8), rng.integers(20, width - 20)
        r = np.hypot(y - cy, x - cx)
        rad = rng.integers(5, 12)
        gap[r <= rad + 2] = rng.integers(0, 4)                  # the wall
        inside = r <= rad - 1
        gap[inside] = rng.integers(150, 250, gap.shape)[inside]  # the pocket
    two = one + gap[..., None] * rng.integers(0, 2, (1, 1, chans)).clip(1)
    return [np.clip(v, 0, 255).astype(dtype) for v in (one, two)]


def with_alpha_holes(pair, seed):
    """Append an alpha channel (255) with zeroed blobs to both images."""
    rng = np.random.default_rng(seed)
    out = []
    for img in pair:
        height, width = img.shape[:2]
        alpha = np.full((height, width), 255, np.int64)
        y, x = np.mgrid[:height, :width]
        for _ in range(5):
            cy, cx = rng.integers(0, height), rng.integers(width // 6, width - width // 6)
            alpha[np.hypot((y - cy) / 1.5, x - cx) <= rng.integers(4, 14)] = 0
        out.append(np.concatenate([img, alpha[..., None].astype(img.dtype)], axis=2))
    return out
