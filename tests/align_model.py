"""The contract of the bracket alignment (include/pano360.h, ``pano_align_mtb``) in NumPy, stage by
stage: Ward's median threshold bitmaps.  Integers throughout, so the device is held to every stage
bit for bit (tests/test_gpu_align.py); the model's own properties are checked in
tests/test_align_host.py."""
import numpy as np

MAX_BITS, EXCLUDE = 6, 4


def levels_for(h, w, max_bits=MAX_BITS):
    """L: the coarsest level keeps a short side of at least 16."""
    return min(max_bits, max(0, int(min(h, w)).bit_length() - 5))


def grey(frame):
    """A: (29 B + 150 G + 77 R + 128) >> 8 of a uint8 BGR frame."""
    f = frame.astype(np.uint32)
    return ((29 * f[..., 0] + 150 * f[..., 1] + 77 * f[..., 2] + 128) >> 8).astype(np.uint8)


def down(g):
    """B: one level up: (a + b + c + d + 2) >> 2 of every whole 2 x 2 block."""
    h, w = g.shape[0] // 2, g.shape[1] // 2
    q = g[:2 * h, :2 * w].astype(np.uint32)
    return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(frame, levels):
    out = [grey(frame)]
    for _ in range(levels):
        out.append(down(out[-1]))
    return out


def median(g):
    """C: the smallest v with #{g <= v} >= (N + 1) // 2, from the 256-bin histogram."""
    cum = np.cumsum(np.bincount(g.ravel(), minlength=256))
    return int(np.argmax(cum >= (g.size + 1) // 2))


def pack(bits):
    """A bool [h][w] image, 32 pixels a uint32 along the row: bit x & 31 of word x >> 5 is pixel x,
    the padding bits 0."""
    h, w = bits.shape
    wpr = (w + 31) // 32
    padded = np.zeros((h, wpr * 32), np.uint8)
    padded[:, :w] = bits
    return np.packbits(padded.reshape(h, wpr, 32), axis=2, bitorder="little").view("<u4").reshape(h, wpr)


def unpack(words, w):
    h = words.shape[0]
    return np.unpackbits(np.ascontiguousarray(words).astype("<u4").view(np.uint8).reshape(h, -1), axis=1,
                         bitorder="little")[:, :w].astype(bool)


def bitmaps(g, m, exclude=EXCLUDE):
    """D: (tb, eb) packed."""
    d = g.astype(np.int32) - m
    return pack(d > 0), pack(np.abs(d) > exclude)


CANDIDATES = ((0, 0),) + tuple((dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0))


def err(a_t, a_e, b_t, b_e, cx, cy):
    """E: the count for candidate (cx, cy) on the unpacked (bool) bitmaps of the reference (a) and
    the frame (b): the pixels of the reference that the shifted frame covers."""
    h, w = a_t.shape
    y0, y1, x0, x1 = max(cy, 0), min(h + cy, h), max(cx, 0), min(w + cx, w)
    if y0 >= y1 or x0 >= x1:
        return 0
    ref = (slice(y0, y1), slice(x0, x1))
    oth = (slice(y0 - cy, y1 - cy), slice(x0 - cx, x1 - cx))
    return int(((a_t[ref] ^ b_t[oth]) & a_e[ref] & b_e[oth]).sum())


def search(ref_maps, maps, widths):
    """E: ``ref_maps`` and ``maps``: [(tb, eb)] packed, per level 0 .. L.  Returns (dx, dy) and the
    uint32 [L + 1][9] counts."""
    L = len(maps) - 1
    counts = np.zeros((L + 1, 9), np.uint32)
    sx = sy = 0
    for l in range(L, -1, -1):
        planes = [unpack(p, widths[l]) for p in ref_maps[l] + maps[l]]
        sx, sy = 2 * sx, 2 * sy
        for i, (dx, dy) in enumerate(CANDIDATES):
            counts[l, i] = err(*planes, sx + dx, sy + dy)
        dx, dy = CANDIDATES[int(np.argmin(counts[l]))]      # (argmin: the first of the smallest)
        sx, sy = sx + dx, sy + dy
    return (sx, sy), counts


def apply(frame, dx, dy):
    """F: aligned[y][x] = src[clamp(y - dy)][clamp(x - dx)]."""
    h, w = frame.shape[:2]
    ys = np.clip(np.arange(h) - dy, 0, h - 1)
    xs = np.clip(np.arange(w) - dx, 0, w - 1)
    return frame[ys][:, xs]


def stages(stack, reference=None, max_bits=MAX_BITS, exclude=EXCLUDE):
    """Every stage of one stack: a dict of ``grey`` [k][L + 1] arrays, ``medians`` int32
    [k][L + 1], ``tb`` / ``eb`` [k][L + 1] packed arrays, ``err`` uint32 [k][L + 1][9] (the
    reference's 0) and ``shifts`` int32 [k][2] = (dx, dy)."""
    k = len(stack)
    r = k // 2 if reference is None else reference
    h, w = stack[0].shape[:2]
    L = levels_for(h, w, max_bits)
    pyr = [pyramid(f, L) for f in stack]
    med = np.array([[median(g) for g in p] for p in pyr], np.int32)
    maps = [[bitmaps(g, int(m), exclude) for g, m in zip(p, ms)] for p, ms in zip(pyr, med)]
    widths = [w >> l for l in range(L + 1)]
    errs = np.zeros((k, L + 1, 9), np.uint32)
    shifts = np.zeros((k, 2), np.int32)
    for i in range(k):
        if i != r:
            shifts[i], errs[i] = search(maps[r], maps[i], widths)
    return {"grey": pyr, "medians": med, "tb": [[t for t, _ in m] for m in maps],
            "eb": [[e for _, e in m] for m in maps], "err": errs, "shifts": shifts}


def shifts(stack, reference=None, max_bits=MAX_BITS, exclude=EXCLUDE):
    return stages(stack, reference, max_bits, exclude)["shifts"]


def align(stack, reference=None, max_bits=MAX_BITS, exclude=EXCLUDE):
    """The aligned stack and its shifts."""
    s = shifts(stack, reference, max_bits, exclude)
    return [apply(f, int(dx), int(dy)) for f, (dx, dy) in zip(stack, s)], s
