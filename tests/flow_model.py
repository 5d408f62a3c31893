"""The local alignment's contract (include/pano360.h, "Local alignment")
restated in NumPy: grey and validity pyramids on the mosaic's grid, the pairs, the block search
coarse to fine, the median smoothing, the field per pixel and the apply.  Everything up to the
block vectors is integer arithmetic; the two float32 stages do one rounding per operation in the
order the header fixes, so the device is held to this model bit for bit at every stage.

A patch is what the blender protocol passes: (warped float32 [h][w][4], mask bool [h][w] with
True = invalid, (slice_y, slice_x) in the mosaic).  ``FAULTS`` switches single rules off for
tests/test_flow_host.py: a model with a fault must break a check."""
import numpy as np

MAX_LEVELS = 4
MIN_COUNT = 128
BLOCK = 16
FAULTS = set()      # of "sign", "alpha", "gain", "count", "median"


class Params:
    def __init__(self, levels=3, gain=16, min_overlap=64):
        self.levels, self.gain, self.min_overlap = levels, gain, min_overlap


def rect_of(patch):
    sy, sx = patch[2]
    return sy.start, sx.start, sy.stop - sy.start, sx.stop - sx.start


def reach(levels):
    return 2 ** (levels + 1) - 1


# ----------------------------------------------------------------- grey, validity, levels
def grey_of(warped, mask):
    """(g uint8, valid bool) of a patch: q_k = uint8(float32(255) * c_k), g = (q0 + 2 q1 + q2 + 2)
    >> 2; an invalid pixel has grey 0."""
    q = (np.float32(255) * warped[..., :3].astype(np.float32)).astype(np.uint8).astype(np.int32)
    g = (q[..., 0] + 2 * q[..., 1] + q[..., 2] + 2) >> 2
    valid = ~np.asarray(mask, bool)
    return np.where(valid, g, 0).astype(np.uint8), valid


def pyramid(patch, shape, levels):
    """[(g uint8, valid bool)] of the levels 0 .. levels over the whole mosaic, its sides rounded
    up to multiples of 16; level l is [Hp >> l][Wp >> l], anchored at the mosaic's origin."""
    H, W = shape
    Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16
    y0, x0, h, w = rect_of(patch)
    g = np.zeros((Hp, Wp), np.uint8)
    v = np.zeros((Hp, Wp), bool)
    g[y0:y0 + h, x0:x0 + w], v[y0:y0 + h, x0:x0 + w] = grey_of(patch[0], patch[1])
    out = [(g, v)]
    for _ in range(levels):
        a = g.astype(np.int32)
        g = ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)
        v = v[0::2, 0::2] & v[0::2, 1::2] & v[1::2, 0::2] & v[1::2, 1::2]
        out.append((g, v))
    return out


def box_of(rect, level):
    """(y0, x0, h, w) in level samples of the part of a camera's pyramid the device stores: the
    rect grown to multiples of 16 mosaic pixels."""
    y0, x0, h, w = rect
    ay0, ax0, ay1, ax1 = y0 & ~15, x0 & ~15, (y0 + h + 15) & ~15, (x0 + w + 15) & ~15
    return ay0 >> level, ax0 >> level, (ay1 - ay0) >> level, (ax1 - ax0) >> level


# ----------------------------------------------------------------------------- pairs
def pairs_for(rects, params):
    """[(i, j, L_ij, y0, y1, x0, x1)]: every i < j whose rects meet in min_overlap x min_overlap."""
    out = []
    for i in range(len(rects)):
        for j in range(i + 1, len(rects)):
            a, b = rects[i], rects[j]
            y0, y1 = max(a[0], b[0]), min(a[0] + a[2], b[0] + b[2])
            x0, x1 = max(a[1], b[1]), min(a[1] + a[3], b[1] + b[3])
            if y1 - y0 < params.min_overlap or x1 - x0 < params.min_overlap:
                continue
            L = min(params.levels, max(0, int(min(y1 - y0, x1 - x0)).bit_length() - 6))
            out.append((i, j, L, y0, y1, x0, x1))
    return out


def block_range(pair, level):
    """(by0, bx0, nby, nbx) of a pair's blocks at a level: those that meet its intersection."""
    _, _, _, y0, y1, x0, x1 = pair
    s = level + 4
    return y0 >> s, x0 >> s, ((y1 - 1) >> s) - (y0 >> s) + 1, ((x1 - 1) >> s) - (x0 >> s) + 1


# ----------------------------------------------------------------------------- search
CANDIDATES = [(0, 0)] + [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]


def sums(gi, vi, gj, vj, by0, bx0, nby, nbx, vec):
    """n and S int64 [9][nby][nbx] of the blocks' candidates; vec int [nby][nbx][2] inherited."""
    hh, ww = gi.shape
    ys = (by0 * 16 + np.arange(nby * 16))[:, None] + np.zeros((1, nbx * 16), np.int64)
    xs = (bx0 * 16 + np.arange(nbx * 16))[None, :] + np.zeros((nby * 16, 1), np.int64)
    inside = (ys < hh) & (xs < ww)
    yc, xc = np.minimum(ys, hh - 1), np.minimum(xs, ww - 1)
    a, va = gi[yc, xc].astype(np.int64), vi[yc, xc] & inside
    vx = np.repeat(np.repeat(vec[..., 0], 16, 0), 16, 1)
    vy = np.repeat(np.repeat(vec[..., 1], 16, 0), 16, 1)
    n = np.zeros((9, nby, nbx), np.int64)
    S = np.zeros((9, nby, nbx), np.int64)
    for k, (dx, dy) in enumerate(CANDIDATES):
        y, x = ys + vy + dy, xs + vx + dx
        ok = (y >= 0) & (y < hh) & (x >= 0) & (x < ww)
        yq, xq = np.clip(y, 0, hh - 1), np.clip(x, 0, ww - 1)
        both = va & ok & vj[yq, xq]
        diff = np.where(both, np.abs(a - gj[yq, xq].astype(np.int64)), 0)
        n[k] = both.reshape(nby, 16, nbx, 16).sum(axis=(1, 3))
        S[k] = diff.reshape(nby, 16, nbx, 16).sum(axis=(1, 3))
    return n, S


def decide(n, S, gain):
    """(offset index int [..], known bool [..]) from n, S int64 [9][..]."""
    need = MIN_COUNT - 1 if "count" in FAULTS else MIN_COUNT
    gain = 0 if "gain" in FAULTS else gain
    elig = n >= need
    w = np.full(n.shape[1:], -1, np.int64)
    Sw, nw = np.zeros_like(S[0]), np.ones_like(n[0])
    for k in range(9):
        better = elig[k] & ((w < 0) | (S[k] * nw < Sw * n[k]))
        w, Sw, nw = np.where(better, k, w), np.where(better, S[k], Sw), np.where(better, n[k], nw)
    known = w >= 0
    moves = 16 * Sw * n[0] + gain * nw * n[0] <= 16 * S[0] * nw
    w = np.where(known & elig[0] & ~moves, 0, w)
    return np.where(known, w, 0), known


def search(pyr_i, pyr_j, pair, params, want_levels=False):
    """The block vectors of a pair: int16 [nby][nbx][4] = (dx, dy, known, 0) at level 0 (or, with
    ``want_levels``, the list of all levels 0 .. L_ij)."""
    L = pair[2]
    levels = [None] * (L + 1)
    for l in range(L, -1, -1):
        by0, bx0, nby, nbx = block_range(pair, l)
        vec = np.zeros((nby, nbx, 2), np.int64)
        if l < L:
            py0, px0, _, _ = block_range(pair, l + 1)
            by = (by0 + np.arange(nby)) >> 1
            bx = (bx0 + np.arange(nbx)) >> 1
            vec = 2 * levels[l + 1][by - py0][:, bx - px0, :2].astype(np.int64)
        n, S = sums(pyr_i[l][0], pyr_i[l][1], pyr_j[l][0], pyr_j[l][1], by0, bx0, nby, nbx, vec)
        w, known = decide(n, S, params.gain)
        off = np.array(CANDIDATES, np.int64)[w]
        out = np.zeros((nby, nbx, 4), np.int16)
        out[..., :2] = vec + off
        out[..., 2] = known
        levels[l] = out
    return levels if want_levels else levels[0]


# -------------------------------------------------------------------------- smoothing
def lower_median(values):
    s = sorted(values)
    return s[len(s) >> 1 if "median" in FAULTS else (len(s) - 1) >> 1]


def smooth(vec):
    """int16 [nby][nbx][2]: the lower median of the known values of the 3 x 3 neighbourhood."""
    nby, nbx = vec.shape[:2]
    out = np.zeros((nby, nbx, 2), np.int16)
    for by in range(nby):
        for bx in range(nbx):
            near = [vec[y, x] for y in range(max(by - 1, 0), min(by + 2, nby))
                    for x in range(max(bx - 1, 0), min(bx + 2, nbx)) if vec[y, x, 2]]
            if vec[by, bx, 2] or len(near) >= 3:
                out[by, bx] = [lower_median([int(v[c]) for v in near]) for c in (0, 1)]
    return out


# ---------------------------------------------------------------------- field per pixel
def lerp(a, b, f):
    return a + f * (b - a)


def field(smoothed, pair, ys, xs):
    """float32 (Fx, Fy) of F_ij at the mosaic pixels ys [:, None] x xs [None, :]."""
    by0, bx0, nby, nbx = block_range(pair, 0)

    def axis(p, lo, n):
        t = (2 * p - 15).astype(np.float32) / np.float32(32)
        b = np.floor(t)
        return (np.clip(b.astype(np.int64), lo, lo + n - 1) - lo,
                np.clip(b.astype(np.int64) + 1, lo, lo + n - 1) - lo, (t - b).astype(np.float32))
    ya, yb, fy = axis(np.asarray(ys), by0, nby)
    xa, xb, fx = axis(np.asarray(xs), bx0, nbx)
    out = []
    for c in (0, 1):
        v = smoothed[..., c].astype(np.float32)
        top = lerp(v[ya][:, xa], v[ya][:, xb], fx[None, :])
        bot = lerp(v[yb][:, xa], v[yb][:, xb], fx[None, :])
        out.append(lerp(top, bot, fy[:, None]))
    return out


# ------------------------------------------------------------------------------ apply
def displacement(patches, c, pairs, fields):
    """float32 (dx, dy) [h][w] of camera c; fields: {pair index: smoothed vectors}."""
    y0, x0, h, w = rect_of(patches[c])
    ys, xs = y0 + np.arange(h), x0 + np.arange(w)

    def cover(k):
        ky0, kx0, kh, kw = rect_of(patches[k])
        al, cov = np.zeros((h, w), np.float32), np.zeros((h, w), bool)
        a0, a1, b0, b1 = max(y0, ky0), min(y0 + h, ky0 + kh), max(x0, kx0), min(x0 + w, kx0 + kw)
        if a0 < a1 and b0 < b1:
            src = np.s_[a0 - ky0:a1 - ky0, b0 - kx0:b1 - kx0]
            dst = np.s_[a0 - y0:a1 - y0, b0 - x0:b1 - x0]
            cov[dst] = ~np.asarray(patches[k][1], bool)[src]
            al[dst] = patches[k][0][..., 3][src]
        return np.where(cov, al, np.float32(0)), cov
    alpha = [cover(k) for k in range(len(patches))]
    W = np.zeros((h, w), np.float32)
    for al, _ in alpha:
        W = W + al
    dx, dy = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    for p, pair in enumerate(pairs):
        if c not in pair[:2]:
            continue
        j = pair[1] if c == pair[0] else pair[0]
        sign = np.float32(-1 if c == pair[1] and "sign" not in FAULTS else 1)
        al, cov = alpha[c if "alpha" in FAULTS else j]
        use = alpha[j][1] & (al > 0)
        fx, fy = field(fields[p], pair, ys, xs)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = al / W
            dx = dx + np.where(use, share * (sign * fx), np.float32(0))
            dy = dy + np.where(use, share * (sign * fy), np.float32(0))
    return dx, dy


def warp_patch(patch, dx, dy):
    """(warped float32 [h][w][4], moved bool [h][w]) of a patch under its displacement."""
    src, mask = patch[0].astype(np.float32), np.asarray(patch[1], bool)
    h, w = mask.shape
    sx = np.arange(w, dtype=np.float32)[None, :] - dx
    sy = np.arange(h, dtype=np.float32)[:, None] - dy
    fx0, fy0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - fx0, sy - fy0
    xa, ya = fx0.astype(np.int64), fy0.astype(np.int64)
    ok = (xa >= 0) & (xa + 1 < w) & (ya >= 0) & (ya + 1 < h)
    xc, yc = np.clip(xa, 0, w - 2) if w > 1 else xa * 0, np.clip(ya, 0, h - 2) if h > 1 else ya * 0
    if w > 1 and h > 1:
        ok &= ~(mask[yc, xc] | mask[yc, xc + 1] | mask[yc + 1, xc] | mask[yc + 1, xc + 1])
    else:
        ok &= False
    moved = ok & ~mask & ((dx != 0) | (dy != 0))
    out = src.copy()
    if moved.any():
        f, g = fx[..., None], fy[..., None]
        top = lerp(src[yc, xc], src[yc, xc + 1], f)
        bot = lerp(src[yc + 1, xc], src[yc + 1, xc + 1], f)
        out[moved] = lerp(top, bot, g)[moved]
    return out, moved


def align(patches, shape, params, want_stages=False):
    """The whole stage: the aligned patches (the masks and slices are the incoming objects; a
    patch with no pair is the incoming tuple) and the stages."""
    rects = [rect_of(p) for p in patches]
    pairs = pairs_for(rects, params)
    top = max([p[2] for p in pairs], default=0)
    pyr = [pyramid(p, shape, top) for p in patches] if pairs else []
    levels = [search(pyr[p[0]], pyr[p[1]], p, params, True) for p in pairs]
    fields = [smooth(lv[0]) for lv in levels]
    out, disp, moved = [], [], []
    for c, patch in enumerate(patches):
        if not any(c in p[:2] for p in pairs):
            out.append(patch)
            disp.append(None)
            moved.append(np.zeros(np.asarray(patch[1]).shape, bool))
            continue
        dx, dy = displacement(patches, c, pairs, fields)
        warped, mv = warp_patch(patch, dx, dy)
        out.append((warped, patch[1], patch[2]))
        disp.append((dx, dy))
        moved.append(mv)
    stages = dict(pairs=pairs, pyramids=pyr, levels=levels, fields=fields, disp=disp, moved=moved)
    return (out, stages) if want_stages else out
