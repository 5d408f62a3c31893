"""Seeded inputs forged for the seam routing (csrc/seam_route.hip), NumPy only: patch sets for
``pano_seam_route_prepare`` and the whole route, plane sets for ``pano_seam_route_flood``.  None
come from images.  The inputs of tests/test_seam_route_host.py (CPU) and
tests/test_gpu_seam_route.py.

``PLANES`` maps a name to ``(a, second, diff, label, group, n, n_groups)``; ``truth`` is the heap
loop on a case (and the classes that labelled a cell in the sweep), computed once.
``PATCHES`` maps a name to ``(patches, shape, ratio)``."""
import functools

import numpy as np

import seam_route_model as sm

TILE = 64                           # the side of the flood's tiles
BATCH = 64                          # PANO_SEAM_BATCH


def marks(n):
    """The cells on either side of every 64-cell border of a line of ``n`` cells."""
    return [m for k in range(1, n // TILE + 1) for m in (TILE * k - 1, TILE * k) if m < n]


def planes_from(a, second, diff, opened, wall, n=None, sparse=False):
    a, second = a.astype(np.int16), second.astype(np.int16)
    label = np.where(wall, sm.WALL, np.where(opened, sm.OPEN, a)).astype(np.int16)
    n = int(max(a.max(), second.max())) + 1 if n is None else n
    if sparse:
        group, n_groups = sm.sparse_groups(a, second, label, n)
    else:
        group, n_groups = sm.groups_of(sm.pairs_of(a, second, label, n))
    # the flood's requirement: the two cameras of an open pixel are of different groups
    o = label == sm.OPEN
    assert (a[o] != second[o]).all() and (group[a[o]] != group[second[o]]).all()
    return a, second, diff.astype(np.uint8), label, group, n, n_groups


def valley(rows, cols, seed, cams, drop=0.35, picket=0.5, step=1):
    """``cams`` territories side by side along x with wavy borders; the cells within a band of a
    border are open for the two cameras it parts.  Levels are low along each border and rise
    towards the band's edges, a share of them dropped to 0, and *pickets*: in every line the
    cells ``64 k - 1`` and ``64 k`` are walls with probability ``picket``, in both directions."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:rows, :cols].astype(np.float64)
    width = cols / cams
    phase = rng.uniform(0, 2 * np.pi, cams)
    pos = x + 0.15 * width * np.sin(2 * np.pi * 1.5 * y / max(rows, 2) + phase[0])
    a = np.clip(np.floor(pos / width), 0, cams - 1).astype(np.int64)
    inside = pos / width - a                            # 0 .. 1 across the territory
    nearer = np.where(inside < 0.5, a - 1, a + 1)
    second = np.where((nearer < 0) | (nearer >= cams), np.where(a == 0, 1, cams - 2), nearer)
    dist = np.minimum(inside, 1 - inside)               # to the nearer border, in territories
    opened = (dist < 0.35) & (nearer >= 0) & (nearer < cams)
    level = 20 + 200 * dist / 0.35
    level = np.floor(level).astype(np.int64) + rng.integers(-30, 31, (rows, cols))
    level = np.clip(level, 3, 255) // step * step
    level[rng.random((rows, cols)) < drop] = 0
    wall = np.zeros((rows, cols), bool)
    for m in marks(cols):
        wall[rng.random(rows) < picket, m] = True
    for m in marks(rows):
        wall[m, rng.random(cols) < picket] = True
    return planes_from(a, second, level, opened, wall, cams)


def serpentine(rows, cols, pitch=2):
    """Open cells for {0, 1} between a seed column of 0 on the left and of 1 on the right: level
    0 but for one corridor of level 255 that winds through the whole grid, a row every ``pitch``
    rows, and that touches the right seeds only.  Class (255, group of 1) has to carry 1 along the
    whole corridor, across every tile border, in both directions."""
    a = np.zeros((rows, cols), np.int64)
    a[:, cols // 2:] = 1
    second = 1 - a
    opened = np.ones((rows, cols), bool)
    opened[:, 0] = opened[:, -1] = False
    level = np.zeros((rows, cols), np.int64)
    lo, hi = 2, cols - 3
    ys = list(range(0, rows, pitch))
    for k, yy in enumerate(ys):
        level[yy, lo:hi + 1] = 255
        if k + 1 < len(ys):
            level[yy:ys[k + 1], lo if k % 2 == 0 else hi] = 255
    level[0, hi + 1:cols - 1] = 255                     # the door: the right seeds' side
    return planes_from(a, second, level, opened, np.zeros((rows, cols), bool), 2)


def three_at_a_point(rows, cols, seed):
    """Three sectors around the centre, every pixel near a border between two of them open for
    those two: all three pairs compete (three groups) and meet in the middle.  Few levels, so that
    fronts of different groups wait in the same class."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:rows, :cols].astype(np.float64)
    angle = np.arctan2(y - rows / 2 + 0.25, x - cols / 2 + 0.25)
    turn = (angle + np.pi) / (2 * np.pi) * 3                # 0 .. 3
    a = np.clip(np.floor(turn), 0, 2).astype(np.int64)
    inside = turn - a
    second = np.where(inside < 0.5, (a - 1) % 3, (a + 1) % 3)
    opened = np.minimum(inside, 1 - inside) < 0.3
    level = rng.choice(np.array([0, 7, 7, 90, 255]), (rows, cols))
    return planes_from(a, second, level, opened, rng.random((rows, cols)) < 0.04, 3)


def same_group_neighbours(rows, cols, seed):
    """Cameras 0 and 2 do not compete (one group), both compete with 1.  The upper half is open
    for {0, 1}, the lower for {2, 1}, so cells that admit 0 lie directly above cells that admit 2
    and both flood in the same class: a fill that joined them would hand one's cells to the
    other."""
    rng = np.random.default_rng(seed)
    a = np.zeros((rows, cols), np.int64)
    a[rows // 2:] = 2
    a[:, 2 * cols // 3:] = 1
    second = np.where(a == 1, np.where(np.arange(rows)[:, None] < rows // 2, 0, 2), 1)
    opened = np.ones((rows, cols), bool)
    opened[:, :2] = opened[:, -2:] = False
    level = rng.choice(np.array([0, 40, 200]), (rows, cols))
    p = planes_from(a, second, level, opened, np.zeros((rows, cols), bool), 3)
    assert p[4].tolist() == [0, 1, 0]
    return p


def far_indices(rows=20, cols=70, seed=5):
    """Cameras 0, 300 and 32000 in three stripes: the labels do not fit a byte."""
    rng = np.random.default_rng(seed)
    ids = np.array([0, 300, 32000])
    stripe = np.minimum(np.arange(cols) * 3 // cols, 2)
    a = np.broadcast_to(ids[stripe], (rows, cols)).copy()
    inside = np.arange(cols) * 3 / cols - stripe
    other = np.where(inside < 0.5, stripe - 1, stripe + 1)
    other = np.where(other < 0, 1, np.where(other > 2, 1, other))
    second = np.broadcast_to(ids[other], (rows, cols)).copy()
    opened = np.broadcast_to((np.minimum(inside, 1 - inside) < 0.3) &
                             (np.arange(cols) > 8) & (np.arange(cols) < cols - 9), (rows, cols))
    level = rng.integers(0, 256, (rows, cols))
    return planes_from(a, second, level, opened, rng.random((rows, cols)) < 0.1, 32001, sparse=True)


def island(rows=40, cols=90, seed=9):
    """A valley with an open island for {3, 4} inside camera 0's seeds (no pixel is labelled 3
    or 4, so nothing reaches it: it keeps a) and a walled-in open pocket for {0, 1}."""
    a, second, diff, label, _, _, _ = valley(rows, cols, seed, 3, picket=0.0)
    a, second, label = a.copy(), second.copy(), label.copy()
    a[5:9, 3:8], second[5:9, 3:8], label[5:9, 3:8] = 3, 4, sm.OPEN
    label[20:27, 2:9] = sm.WALL
    a[21:26, 3:8], second[21:26, 3:8], label[21:26, 3:8] = 0, 1, sm.OPEN
    return planes_from(a, second, diff, label == sm.OPEN, label == sm.WALL, 5)


def transposed(p):
    a, second, diff, label, group, n, n_groups = p
    return (np.ascontiguousarray(a.T), np.ascontiguousarray(second.T),
            np.ascontiguousarray(diff.T), np.ascontiguousarray(label.T), group, n, n_groups)


PLANES = {
    "valley-65x129": valley(65, 129, 1, 4),
    "valley-63x127": valley(63, 127, 2, 3),
    "valley-130x70": valley(130, 70, 3, 3),
    "valley-70x130-step64": valley(70, 130, 4, 5, step=64),
    "valley-1x700": valley(1, 700, 5, 5, drop=0.1),
    "valley-700x1": transposed(valley(1, 700, 6, 4, drop=0.1)),
    "serpentine-130x200": serpentine(130, 200),
    "serpentine-200x130": transposed(serpentine(130, 200)),
    "three-at-a-point-67x90": three_at_a_point(67, 90, 7),
    "same-group-neighbours-40x70": same_group_neighbours(40, 70, 8),
    "far-indices-20x70": far_indices(),
    "island-40x90": island(),
}
SERPENTINES = ("serpentine-130x200", "serpentine-200x130")


@functools.lru_cache(maxsize=None)
def truth(name):
    """(the heap loop's label plane, the owner map, the classes that labelled a cell in the
    sweep), read-only."""
    a, second, diff, label, group, _, _ = PLANES[name]
    heap = sm.flood_heap(a, second, diff, label, group)
    sweep, worked = sm.flood_sweep(a, second, diff, label, group, want_stats=True)
    assert np.array_equal(sweep, heap), name
    owner = sm.finish(a, heap)
    heap.setflags(write=False)
    owner.setflags(write=False)
    return heap, owner, worked


# ---- patch sets -------------------------------------------------------------------------------
def hat(size):
    t = np.arange(size, dtype=np.float64)
    return 1 - np.abs(2 * (t + 0.5) / size - 1)


def forged_patches(shape, rects, seed, steps=8, holes=3):
    """Patches of the blender protocol at ``rects`` (y0, y1, x0, x1): alpha a hat product
    quantised to ``steps`` levels (ties between cameras), colours k / 255 exactly for half the
    pixels and anything in [0, 1] for the rest, masked holes (alpha 0 under them), and a few
    masked pixels that keep their alpha (invalid where nothing else covers them: walls)."""
    rng = np.random.default_rng(seed)
    patches = []
    for y0, y1, x0, x1 in rects:
        h, w = y1 - y0, x1 - x0
        warped = np.zeros((h, w, 4), np.float32)
        exact = (rng.integers(0, 256, (h, w, 3)).astype(np.float32) / np.float32(255))
        loose = rng.random((h, w, 3)).astype(np.float32)
        warped[..., :3] = np.where(rng.random((h, w, 1)) < 0.5, exact, loose)
        alpha = np.outer(hat(h), hat(w))
        warped[..., 3] = (np.ceil(alpha * steps) / steps).astype(np.float32)
        mask = np.zeros((h, w), bool)
        for _ in range(holes):
            yy, xx = int(rng.integers(0, h)), int(rng.integers(0, w))
            mask[yy:yy + int(rng.integers(1, 9)), xx:xx + int(rng.integers(1, 9))] = True
        warped[..., 3][mask] = 0
        stray = rng.random((h, w)) < 0.002
        mask |= stray
        patches.append((warped, mask, np.s_[y0:y1, x0:x1]))
    return patches


def _prepare_cases():
    out = {}
    # three cameras side by side, the middle one short
    out["3-on-63x127"] = (forged_patches((63, 127), [(0, 63, 0, 70), (5, 50, 40, 100),
                                                     (0, 63, 75, 127)], 11), (63, 127), 0.5)
    # four cameras over one region (a pixel covered by four), ratio 1: only exact ties are open
    out["4-on-65x129"] = (forged_patches((65, 129), [(0, 65, 0, 80), (0, 60, 30, 110),
                                                     (10, 65, 50, 129), (20, 50, 40, 90)], 12,
                                         steps=4), (65, 129), 1.0)
    # five cameras, two of them the same rectangle (ties everywhere between them), wide zones
    out["5-on-130x66"] = (forged_patches((130, 66), [(0, 60, 0, 66), (30, 100, 0, 50),
                                                     (30, 100, 0, 50), (70, 130, 10, 66),
                                                     (50, 90, 20, 60)], 13), (130, 66), 0.25)
    return out


PATCHES = _prepare_cases()


def ghost_pair(shape=(70, 150), rect=(20, 50, 72, 78)):
    """Two patches whose colours are the same function of the mosaic position, but for a
    rectangle of another colour in the first one only, across the argmax seam (x = 75) and well
    inside the zone ratio 0.5 opens (x = 67 .. 83)."""
    H, W = shape
    y, x = np.mgrid[:H, :W].astype(np.float32)
    scene = np.stack([x / W, y / H, (x + y) / (W + H)], axis=-1).astype(np.float32)
    patches = []
    for x0, x1 in ((0, 100), (50, 150)):
        warped = np.zeros((H, x1 - x0, 4), np.float32)
        warped[..., :3] = scene[:, x0:x1]
        warped[..., 3] = np.outer(hat(H), hat(x1 - x0)).astype(np.float32)
        patches.append((warped, np.zeros((H, x1 - x0), bool), np.s_[0:H, x0:x1]))
    y0, y1, xa, xb = rect
    patches[0][0][y0:y1, xa:xb, :3] = np.float32([0.9, 0.1, 0.8])
    return patches, shape, 0.5
