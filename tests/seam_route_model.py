"""NumPy restatement of the seam routing in front of the multiband blend (``-b seam``;
include/pano360.h, "Seam routing").  The truth of every seam-route test.

Input: the patches of the blender protocol, ``(warped float32 [h][w][4], mask bool [h][w],
(row slice, column slice))``, alpha = ``warped[..., 3]``, and the mosaic's shape.

1. ``a``, ``valid``: first-index argmax of alpha (-1 where every alpha is 0), OR of ``~mask``.
2. ``b``: the camera other than ``a`` with the largest alpha > 0, lowest index on ties, else -1.
3. ``D``: where b >= 0, max over the colour channels of |qa - qb|, q = uint8(float32(255) c).
4. open: valid, a >= 0, b >= 0 and alpha_b >= float32(ratio) alpha_a (one float32 product).
   The other valid pixels with a >= 0 are seeds (label a), the rest walls.
   Label plane: a on seeds, OPEN on open pixels, WALL on walls.
5. Two cameras compete when an open pixel has them as {a, b}; ``group[c]`` is the smallest
   non-negative integer no lower-indexed competitor of c uses.
6. The flood, as the literal heap loop (``flood_heap``) and as the class sweep (``flood_sweep``):
   d = 255 .. 0, g = 0 .. G - 1, every camera c of group g: each 4-connected component of
   unlabelled open pixels with D >= d that admit c (c is their a or their b) and that touches a
   pixel labelled c becomes c.
7. owner: the label, a where an open pixel was never reached, -1 on walls.

``flood_sweep`` also takes four faults (8-connectivity, ``D > d``, reversed group order, no
admissibility): the host test shows that each changes labels on the forged grids, so that a
device flood with one of them cannot pass."""
import heapq

import numpy as np

OPEN, WALL = -1, -2


# ---- steps 1 - 4 --------------------------------------------------------------------------------
def stack(patches, shape):
    """(covered bool [n][H][W], alpha float32 [n][H][W], colour float32 [n][H][W][3],
    unmasked bool [n][H][W]) of the patches on the mosaic."""
    n = len(patches)
    covered = np.zeros((n,) + tuple(shape), bool)
    alpha = np.zeros((n,) + tuple(shape), np.float32)
    colour = np.zeros((n,) + tuple(shape) + (3,), np.float32)
    unmasked = np.zeros((n,) + tuple(shape), bool)
    for i, (warped, mask, irange) in enumerate(patches):
        covered[i][irange] = True
        alpha[i][irange] = warped[..., 3]
        colour[i][irange] = warped[..., :3]
        unmasked[i][irange] = ~np.asarray(mask, bool)
    return covered, alpha, colour, unmasked


def ownership(patches, shape):
    """(a int16 [H][W], valid bool [H][W]): what ``pano_ownership`` computes."""
    _, alpha, _, unmasked = stack(patches, shape)
    a = np.where(alpha.max(axis=0) > 0, alpha.argmax(axis=0), -1).astype(np.int16)
    return a, unmasked.any(axis=0)


def quant(colour):
    return (np.float32(255) * colour.astype(np.float32)).astype(np.uint8)


def prepare(patches, shape, ratio):
    """Steps 1 - 4: a dict of a, valid, second, diff, label, open, pairs (uint8 [n][n]) and
    present (uint8 [256])."""
    n = len(patches)
    _, alpha, colour, unmasked = stack(patches, shape)
    a, valid = ownership(patches, shape)
    index = np.arange(n).reshape(n, 1, 1)
    others = np.where(index == a[None], np.float32(0), alpha)
    second = np.where(others.max(axis=0) > 0, others.argmax(axis=0), -1).astype(np.int16)

    def take(plane, who):
        return np.take_along_axis(plane, np.maximum(who, 0).astype(np.int64)[None], axis=0)[0]
    both = (a >= 0) & (second >= 0)
    q = quant(colour).astype(np.int32)
    qa = np.take_along_axis(q, np.maximum(a, 0).astype(np.int64)[None, ..., None], axis=0)[0]
    qb = np.take_along_axis(q, np.maximum(second, 0).astype(np.int64)[None, ..., None], axis=0)[0]
    diff = np.where(both, np.abs(qa - qb).max(axis=-1), 0).astype(np.uint8)
    alpha_a, alpha_b = take(alpha, a), take(alpha, second)
    bar = np.float32(ratio) * alpha_a                       # one float32 product
    assert bar.dtype == np.float32
    opened = valid & both & (alpha_b >= bar)
    label = np.where(valid & (a >= 0), np.where(opened, OPEN, a), WALL).astype(np.int16)
    pairs = np.zeros((n, n), np.uint8)
    pairs[a[opened], second[opened]] = 1
    present = np.zeros(256, np.uint8)
    present[diff[opened]] = 1
    return dict(a=a, valid=valid, second=second, diff=diff, label=label, open=opened, pairs=pairs,
                present=present)


# ---- step 5 -----------------------------------------------------------------------------------
def pairs_of(a, second, label, n):
    """The pair matrix of forged planes."""
    pairs = np.zeros((n, n), np.uint8)
    opened = label == OPEN
    pairs[a[opened], second[opened]] = 1
    return pairs


def groups_of(pairs):
    """(group int32 [n], number of groups): greedy colouring in index order."""
    n = len(pairs)
    compete = (pairs | pairs.T).astype(bool)
    group = np.zeros(n, np.int32)
    for c in range(n):
        used = set(group[:c][compete[c, :c]].tolist())
        k = 0
        while k in used:
            k += 1
        group[c] = k
    return group, int(group.max()) + 1 if n else 1


def sparse_groups(a, second, label, n):
    """``groups_of`` for forged planes whose camera indices are few but large: the cameras that
    occur are coloured, every other one gets group 0."""
    opened = label == OPEN
    cams = np.unique(np.concatenate([a[opened], second[opened], label[label >= 0]])).tolist()
    small = np.zeros((len(cams), len(cams)), np.uint8)
    at = {c: k for k, c in enumerate(cams)}
    for x, y in set(zip(a[opened].tolist(), second[opened].tolist())):
        small[at[x], at[y]] = 1
    g, count = groups_of(small)
    group = np.zeros(n, np.int32)
    group[cams] = g
    return group, count


# ---- step 6 -----------------------------------------------------------------------------------
STEPS4 = ((0, 1), (0, -1), (1, 0), (-1, 0))


def flood_heap(a, second, diff, label, group):
    """The literal loop: pop the smallest (-D, group[c], c, y, x), label the pixel if it is still
    unlabelled, push its unlabelled open 4-neighbours that admit c.  Returns the label plane."""
    rows, cols = label.shape
    lab = label.astype(np.int64).tolist()
    first, other, level = a.tolist(), second.tolist(), diff.astype(np.int64).tolist()
    grp = np.asarray(group).tolist()
    heap = []

    def spread(y, x, c):
        for dy, dx in STEPS4:
            ny, nx = y + dy, x + dx
            if 0 <= ny < rows and 0 <= nx < cols and lab[ny][nx] == OPEN and \
                    c in (first[ny][nx], other[ny][nx]):
                heapq.heappush(heap, (-level[ny][nx], grp[c], c, ny, nx))
    for y in range(rows):
        for x in range(cols):
            if lab[y][x] >= 0:
                spread(y, x, lab[y][x])
    while heap:
        _, _, c, y, x = heapq.heappop(heap)
        if lab[y][x] != OPEN:
            continue
        lab[y][x] = c
        spread(y, x, c)
    return np.array(lab, np.int16).reshape(rows, cols)


def _touching(has, connect8):
    """Cells with a neighbour in ``has``."""
    out = np.zeros_like(has)
    out[1:] |= has[:-1]
    out[:-1] |= has[1:]
    out[:, 1:] |= has[:, :-1]
    out[:, :-1] |= has[:, 1:]
    if connect8:
        out[1:, 1:] |= has[:-1, :-1]
        out[1:, :-1] |= has[:-1, 1:]
        out[:-1, 1:] |= has[1:, :-1]
        out[:-1, :-1] |= has[1:, 1:]
    return out


def flood_sweep(a, second, diff, label, group, want_stats=False, connect8=False, strict=False,
                reverse_groups=False, ignore_admissible=False):
    """The class sweep; with ``want_stats`` also the number of classes (d, g) that labelled a
    cell.  The four switches are the faults of the module docstring."""
    from scipy import ndimage
    lab = label.astype(np.int16).copy()
    group = np.asarray(group)
    opened = lab == OPEN
    cams = np.unique(np.concatenate([a[opened], second[opened]]))
    cams = cams[cams >= 0]
    n_groups = int(group[cams].max()) + 1 if len(cams) else 0
    order = range(n_groups - 1, -1, -1) if reverse_groups else range(n_groups)
    structure = np.ones((3, 3), bool) if connect8 else None
    worked = 0
    for d in np.unique(diff[opened])[::-1] if opened.any() else ():
        for g in order:
            did = False
            for c in cams[group[cams] == g].tolist():
                free = (lab == OPEN) & ((diff > d) if strict else (diff >= d))
                if not ignore_admissible:
                    free &= (a == c) | (second == c)
                front = free & _touching(lab == c, connect8)
                if not front.any():
                    continue
                comp, _ = ndimage.label(free, structure=structure)
                lab[np.isin(comp, np.unique(comp[front]))] = c
                did = True
            worked += did
    return (lab, worked) if want_stats else lab


# ---- step 7 and the whole ---------------------------------------------------------------------
def finish(a, label):
    return np.where(label >= 0, label, np.where(label == OPEN, a, -1)).astype(np.int16)


def route(patches, shape, ratio, flood=flood_heap):
    """The whole contract: (owner int16 [H][W], valid bool [H][W], the ``prepare`` dict with
    ``group``, ``n_groups`` and the flooded ``flooded`` plane added)."""
    p = prepare(patches, shape, ratio)
    p["group"], p["n_groups"] = groups_of(p["pairs"])
    p["flooded"] = flood(p["a"], p["second"], p["diff"], p["label"], p["group"])
    return finish(p["a"], p["flooded"]), p["valid"], p


def seam_pairs(owner):
    """(bool [H][W]) pixels with a 4-neighbour of another owner, both owned."""
    out = np.zeros(owner.shape, bool)
    for sl_a, sl_b in ((np.s_[1:], np.s_[:-1]), (np.s_[:, 1:], np.s_[:, :-1])):
        differ = (owner[sl_a] != owner[sl_b]) & (owner[sl_a] >= 0) & (owner[sl_b] >= 0)
        out[sl_a] |= differ
        out[sl_b] |= differ
    return out
