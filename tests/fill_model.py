"""The pull-push fill of include/pano360.h (pano_fill_u8) in float64 NumPy: what csrc/fill.hip
computes in float32.  ``fill`` returns the uint8 result and f_0, the filled level 0 before
rounding; ``near_tie`` says where float32 may round f_0 to the other side of a half."""
import numpy as np

TIE_BAND = 4e-3                     # |f_0 - (k + 0.5)| below this: the comparison allows 1 level


def level_shapes(h, w):
    shapes = [(int(h), int(w))]
    while shapes[-1] != (1, 1):
        a, b = shapes[-1]
        shapes.append(((a + 1) // 2, (b + 1) // 2))
    return shapes


def pull(img, mask):
    """([c_l], [v_l]): float64 [H_l][W_l][3] colours and bool [H_l][W_l] validities of every level."""
    c, v = [np.asarray(img, np.float64)], [np.asarray(mask) != 0]
    while c[-1].shape[:2] != (1, 1):
        h, w = v[-1].shape
        ph, pw = h + (h & 1), w + (w & 1)           # children outside the level: invalid
        cc = np.zeros((ph, pw, 3))
        vv = np.zeros((ph, pw), bool)
        cc[:h, :w], vv[:h, :w] = c[-1], v[-1]
        total = np.zeros((ph // 2, pw // 2, 3))
        count = np.zeros((ph // 2, pw // 2))
        for dy in (0, 1):                           # (0,0), (0,1), (1,0), (1,1)
            for dx in (0, 1):
                child_v = vv[dy::2, dx::2]
                total = total + np.where(child_v[..., None], cc[dy::2, dx::2], 0.0)
                count = count + child_v
        c.append(np.where(count[..., None] > 0, total / np.maximum(count, 1)[..., None], 0.0))
        v.append(count > 0)
    return c, v


def push(c, v, closed):
    """f_0: every level's invalid pixels filled from the level above, from the top down."""
    f = c[-1]
    for l in range(len(c) - 2, -1, -1):
        h, w = v[l].shape
        uh, uw = v[l + 1].shape
        y, x = np.arange(h)[:, None], np.arange(w)[None, :]
        Y, X = y >> 1, x >> 1
        Y2 = np.clip(Y + np.where(y & 1, 1, -1), 0, uh - 1)
        X2 = X + np.where(x & 1, 1, -1)
        X2 = X2 % uw if closed else np.clip(X2, 0, uw - 1)
        g = ((0.5625 * f[Y, X] + 0.1875 * f[Y, X2]) + 0.1875 * f[Y2, X]) + 0.0625 * f[Y2, X2]
        f = np.where(v[l][..., None], c[l], g)
    return f


def fill(img, mask, closed=False):
    """(uint8 [H][W][3] result, float64 f_0) of an image uint8 [H][W][3] and a mask [H][W]."""
    img = np.asarray(img)
    valid = np.asarray(mask) != 0
    c, v = pull(img, valid)
    f0 = push(c, v, closed)
    if not valid.any():
        return img.copy(), f0
    rounded = np.clip(np.floor(f0 + 0.5), 0, 255).astype(np.uint8)
    return np.where(valid[..., None], img, rounded), f0


def near_tie(f0):
    """bool, per value: f_0 within ``TIE_BAND`` of k + 0.5."""
    return np.abs(f0 - np.floor(f0) - 0.5) < TIE_BAND


def blobs(h, w, n, r, seed=0):
    """A uint8 [h][w] mask, 1 = valid, with n discs of radius up to r cut out at seeded places."""
    rng = np.random.default_rng(seed)
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    mask = np.ones((h, w), np.uint8)
    for _ in range(n):
        cy, cx, rad = rng.integers(0, h), rng.integers(0, w), rng.uniform(0.5, r)
        mask[(y - cy) ** 2 + (x - cx) ** 2 <= rad * rad] = 0
    return mask
