"""The contract of the bracket deghosting (include/pano360.h, ``pano_deghost_u8``) in NumPy, stage
by stage: a pixel of an exposure whose brightness RANK within its own frame disagrees with the
reference exposure's shows other scene content, and is replaced by the reference's pixel carried to
the exposure's brightness through the histogram-matching map of the two frames.  Integers
throughout, so the device is held to every stage bit for bit (tests/test_gpu_deghost.py); the
model's own properties are checked in tests/test_deghost_host.py."""
import numpy as np

from align_model import grey, pack, unpack  # noqa: F401  (stage A's grey and the bitmaps' packing are align's)

SLACK, TOL, ERODE, DILATE = 3, 8, 1, 3


def hists(frame):
    """A: uint32 [4][256], the counts of g, B, G and R."""
    planes = [grey(frame), frame[..., 0], frame[..., 1], frame[..., 2]]
    return np.stack([np.bincount(p.ravel(), minlength=256) for p in planes]).astype(np.uint32)


def below(hist):
    """B: below[v] = #{. < v} for v = 0 .. 256, as Python-sized integers."""
    return np.concatenate(([0], np.cumsum(hist.astype(np.int64))))


def ranks(hist_g, slack=SLACK):
    """B: uint8 [2][256]: lo[v] = below[max(v - slack, 0)] 255 // N, hi[v] = below[min(v + slack + 1,
    256)] 255 // N - the interval of ranks, in 1/255, that a grey value v and its ``slack``
    neighbours on both sides cover."""
    b = below(hist_g)
    n = int(b[256])
    out = np.zeros((2, 256), np.uint8)
    for v in range(256):
        out[0, v] = int(b[max(v - slack, 0)]) * 255 // n
        out[1, v] = int(b[min(v + slack + 1, 256)]) * 255 // n
    return out


def colour_map(hist_i, hist_r):
    """B: uint8 [256]: value v of the reference's channel -> the smallest u with
    below_i[u + 1] >= below_r[v] + (hist_r[v] + 1) // 2: the value of frame i at the rank of the
    middle of the reference's bin."""
    bi, br = below(hist_i), below(hist_r)
    out = np.zeros(256, np.uint8)
    for v in range(256):
        target = int(br[v]) + (int(hist_r[v]) + 1) // 2
        out[v] = int(np.argmax(bi[1:] >= target))
    return out


def raw_mask(g_i, g_r, ranks_i, ranks_r, tol=TOL):
    """C: bool [h][w]: the rank intervals of the two pixels are more than ``tol`` apart."""
    lo_i, hi_i = ranks_i[0].astype(np.int32)[g_i], ranks_i[1].astype(np.int32)[g_i]
    lo_r, hi_r = ranks_r[0].astype(np.int32)[g_r], ranks_r[1].astype(np.int32)[g_r]
    return (lo_i > hi_r + tol) | (lo_r > hi_i + tol)


def _window(bits, radius, outside, fold):
    h, w = bits.shape
    padded = np.full((h + 2 * radius, w + 2 * radius), outside, bool)
    padded[radius:radius + h, radius:radius + w] = bits
    # (the padding is one value, so the square folds as rows of columns; the direct per-pixel
    # window is what tests/test_deghost_host.py compares this with)
    rows = padded[:, radius:radius + w].copy()
    for dx in range(2 * radius + 1):
        rows = fold(rows, padded[:, dx:dx + w])
    out = rows[radius:radius + h].copy()
    for dy in range(2 * radius + 1):
        out = fold(out, rows[dy:dy + h])
    return out


def erode(bits, radius):
    """D: set where the whole (2 radius + 1)^2 square is set; pixels outside the image count as set."""
    return _window(bits, radius, True, np.logical_and)


def dilate(bits, radius):
    """D: set where any pixel of the square is; pixels outside the image count as clear."""
    return _window(bits, radius, False, np.logical_or)


def clean(bits, erode_by=ERODE, dilate_by=DILATE):
    return dilate(erode(bits, erode_by), dilate_by)


def apply(frame, ref, mask, maps):
    """E: dst[y][x][c] = mask ? map_c[ref[y][x][c]] : src[y][x][c]."""
    out = frame.copy()
    for c in range(3):
        out[..., c] = np.where(mask, maps[c][ref[..., c]], frame[..., c])
    return out


def stages(stack, reference=None, slack=SLACK, tol=TOL, erode_by=ERODE, dilate_by=DILATE):
    """Every stage of one stack: ``hists`` uint32 [k][4][256], ``ranks`` uint8 [k][2][256], ``maps``
    uint8 [k][3][256] (the reference's is the identity), ``raw`` and ``mask`` [k] packed uint32
    [h][wpr] (the reference's 0), ``counts`` int32 [k] and ``out``: the frames, a changed exposure
    a new array, the reference and every exposure with a count of 0 the array that came in."""
    k = len(stack)
    r = k // 2 if reference is None else reference
    h, w = stack[0].shape[:2]
    hs = np.stack([hists(f) for f in stack])
    rk = np.stack([ranks(x[0], slack) for x in hs])
    greys = [grey(f) for f in stack]
    maps = np.zeros((k, 3, 256), np.uint8)
    raws, masks, out = [], [], []
    counts = np.zeros(k, np.int32)
    for i in range(k):
        if i == r:
            maps[i] = np.arange(256, dtype=np.uint8)
            raws.append(pack(np.zeros((h, w), bool))), masks.append(pack(np.zeros((h, w), bool)))
            out.append(stack[i])
            continue
        maps[i] = [colour_map(hs[i][1 + c], hs[r][1 + c]) for c in range(3)]
        raw = raw_mask(greys[i], greys[r], rk[i], rk[r], tol)
        mask = clean(raw, erode_by, dilate_by)
        counts[i] = int(mask.sum())
        raws.append(pack(raw)), masks.append(pack(mask))
        out.append(apply(stack[i], stack[r], mask, maps[i]) if counts[i] else stack[i])
    return {"hists": hs, "ranks": rk, "maps": maps, "raw": raws, "mask": masks, "counts": counts, "out": out}


def deghost(stack, reference=None, slack=SLACK, tol=TOL, erode_by=ERODE, dilate_by=DILATE):
    """The deghosted stack and the counts."""
    s = stages(stack, reference, slack, tol, erode_by, dilate_by)
    return s["out"], s["counts"]
