"""The contract of the multiband collapse (pano_multiband_compose, csrc/blend.hip, without
interior map and level classes) restated in NumPy float32.

Every operation below runs on float32 arrays, one rounding each, in the order the reference sums
(stitcher.py:227-241): the records in table order, per record the levels ascending.  The kernel
is plain float32 arithmetic in that order (the library builds with -ffp-contract=off), so it is
held to this model bit for bit; tests/test_compose_host.py holds the model to the oracle's
``multiband_blend`` bit for bit.

A record's ``planes`` / ``blurred`` fields hold OFFSETS in floats into the two arenas (what
pano_layout_windows leaves in them before pano_layout_place)."""
import numpy as np

F32 = np.float32


def window(records, planes, i):
    """Colour planes of record i over its window V: a [3][vh][vpitch] view into the arena."""
    r = records[i]
    vh, vp, off = int(r["vh"]), int(r["vpitch"]), int(r["planes"])
    return planes[off:off + 3 * vh * vp].reshape(3, vh, vp)


def copies(records, blurred, i, n_blur):
    """Blurred copies of record i over its rectangle A: a [n_blur][4][ah][apitch] view."""
    r = records[i]
    ah, ap, off = int(r["ah"]), int(r["apitch"]), int(r["blurred"])
    return blurred[off:off + n_blur * 4 * ah * ap].reshape(n_blur, 4, ah, ap)


def area(r):
    """Rectangle A of a record in mosaic coordinates: (row slice, column slice)."""
    gy, gx = int(r["y0"]) + int(r["ay0"]), int(r["x0"]) + int(r["ax0"])
    return slice(gy, gy + int(r["ah"])), slice(gx, gx + int(r["aw"]))


def collapse(records, planes, blurred, owner, valid, shape, strip, n_levels, stats=None):
    """(float32 [H][W][3], uint8 [H][W][3]) of the collapse; only the columns [xs0, xs1) of
    ``strip`` are produced, the others are 0.  ``stats`` (a dict, optional) receives what the
    case conditions are judged on: ``m`` int [H][W] = the records over a pixel, ``zero`` bool
    [H][W] = some level's weight sum is 0 under at least one record, ``raw`` float32 [H][W][3] =
    the sum of the levels before it is clipped."""
    H, W = shape
    xs0, xs1 = strip
    L = int(n_levels)
    layer = np.zeros((L, H, W, 3), F32)
    wsum = np.zeros((L, H, W), F32)
    m = np.zeros((H, W), np.int64)
    for i in range(len(records)):                           # table order
        r = records[i]
        ys, xs = area(r)                                    # only inside rectangle A
        ah, aw = int(r["ah"]), int(r["aw"])
        oy, ox = int(r["ay0"]) - int(r["vy0"]), int(r["ax0"]) - int(r["vx0"])
        hi = window(records, planes, i)[:, oy:oy + ah, ox:ox + aw]
        b = copies(records, blurred, i, L - 1)[..., :aw] if L > 1 else None
        ha = (owner[ys, xs] == int(r["index"])).astype(F32)             # sharp alpha (:208)
        for k in range(L):
            if k < L - 1:
                g, a = b[k, :3], b[k, 3]
                rgb = hi - g                                            # :227
                hi, ha = g, a                                           # :229
            else:
                rgb, a = hi, ha
            prod = (rgb * a[None]).astype(F32).transpose(1, 2, 0)
            layer[k][ys, xs] = layer[k][ys, xs] + prod                  # :231
            wsum[k][ys, xs] = wsum[k][ys, xs] + a                       # :232
        m[ys, xs] += 1
    ok = (np.asarray(valid) != 0)[..., None]
    out = np.zeros((H, W, 3), F32)
    for k in range(L):
        ws = np.where(wsum[k] == F32(0), F32(1), wsum[k])[..., None]    # :237
        out = out + np.where(ok, layer[k], F32(0)) / ws                 # :236, 238
    assert out.dtype == F32
    v = np.where(out < F32(0), F32(0), np.where(out > F32(1), F32(1), out))   # :240
    u8 = (F32(255) * v).astype(np.uint8)                                # :241, truncation
    if stats is not None:
        stats["m"] = m
        stats["zero"] = (m > 0) & (wsum == F32(0)).any(axis=0)
        stats["raw"] = out
    v[:, :xs0], v[:, xs1:] = 0, 0
    u8[:, :xs0], u8[:, xs1:] = 0, 0
    return v, u8


def records_over(records, y, x):
    """Table positions of the records whose rectangle A holds mosaic pixel (y, x)."""
    hit = []
    for i in range(len(records)):
        ys, xs = area(records[i])
        if ys.start <= y < ys.stop and xs.start <= x < xs.stop:
            hit.append(i)
    return hit
