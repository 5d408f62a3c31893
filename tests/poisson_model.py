"""Float64 restatement of the two linear operators behind the reference's
``blend.poisson_blend`` (blend.py:143-203), written from their observed behaviour and pinned to
the reference by the products stored in tests/golden/poisson_*.npz.

Flat row-major indices: ``i = y * W + x``, ``N = H * W``.  Both operators link pixel ``i`` to
``n`` in ``{i-1, i+1, i-W, i+W}`` with ``0 <= n < N`` - flat neighbours, so the last pixel of a
row and the first of the next are "left" and "right" of each other - minus what the reference's
zeroed diagonal slots drop:

``P`` (the right-hand side's operator, ``poisson_matrix(W, H)``): 4 on the diagonal, -1 at every
  flat neighbour whose column is not ``W-1``.  Nobody reads the last column; a last-column pixel
  reads its left neighbour and the first pixel of the next row only.
``A`` (the system, ``poisson_matrix(W, H, positions)``): identity rows outside the mask; a mask
  row has 4 on the diagonal and -1 at its flat neighbours, without ``i+1`` when ``x == W-2`` and
  without ``i-1`` when ``x == 0``.  A mask pixel at ``x == W-1`` keeps ``i+1`` (a wrap link) and
  both vertical neighbours.  ``A`` is not symmetric.

``links(H, W, system)`` states both rules once; ``rhs``, ``apply_P``, ``apply_A`` and
``matrix_A`` (a SciPy CSR, for CPU solves in the tests) all go through it.
"""
import numpy as np


def links(H, W, system):
    """For each of the four flat offsets (-1, +1, -W, +W): (offset, bool[N] "row i has this
    link").  ``system`` False: the links of P; True: those of a mask row of A."""
    N = H * W
    i = np.arange(N)
    x = i % W
    out = []
    for off in (-1, 1, -W, W):
        n = i + off
        keep = (n >= 0) & (n < N)
        if system:
            if off == 1:
                keep &= x != W - 2
            if off == -1:
                keep &= x != 0
        else:
            keep &= (n % W) != W - 1
        out.append((off, keep))
    return out


def _apply(v, H, W, system, rows=None):
    """(4 v[i] - sum of linked v[n]) per row; rows: bool[N], the others are identity rows."""
    v = np.asarray(v, np.float64).reshape(-1)
    N = H * W
    out = 4.0 * v
    for off, keep in links(H, W, system):
        src = np.clip(np.arange(N) + off, 0, N - 1)
        out = out - np.where(keep, v[src], 0.0)
    if rows is not None:
        out = np.where(rows, out, v)
    return out


def apply_P(v, H, W):
    """``poisson_matrix(W, H) @ v`` for a flat float64 vector."""
    return _apply(v, H, W, False)


def apply_A(x, mask):
    """``poisson_matrix(W, H, positions) @ x``; mask: [H][W], nonzero selects the mask rows."""
    H, W = mask.shape
    return _apply(x, H, W, True, (np.asarray(mask) != 0).reshape(-1))


def rhs(src, tgt, mask):
    """b of one channel: P . src inside the mask, tgt outside.  src, tgt: [H][W]."""
    H, W = mask.shape
    inside = (np.asarray(mask) != 0).reshape(-1)
    b = apply_P(np.asarray(src, np.float64).reshape(-1), H, W)
    return np.where(inside, b, np.asarray(tgt, np.float64).reshape(-1))


def matrix_A(mask):
    """A as a SciPy CSR matrix (tests only; the product does not depend on SciPy)."""
    import scipy.sparse as sp
    H, W = mask.shape
    N = H * W
    inside = (np.asarray(mask) != 0).reshape(-1)
    i = np.arange(N)
    rows, cols, vals = [i], [i], [np.where(inside, 4.0, 1.0)]
    for off, keep in links(H, W, True):
        sel = inside & keep
        rows.append(i[sel])
        cols.append(i[sel] + off)
        vals.append(np.full(int(sel.sum()), -1.0))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                         shape=(N, N))


def solve(src, tgt, mask):
    """The float64 solution per channel, [C][H][W], by SciPy's direct sparse solver (SuperLU,
    what the reference's spsolve runs; A is factorised once for all channels), and the image
    the reference would return: clip to 0..255, truncate to the target's dtype."""
    from scipy.sparse.linalg import splu
    H, W = mask.shape
    lu = splu(matrix_A(mask).tocsc())
    sols = np.stack([lu.solve(rhs(src[..., c], tgt[..., c], mask)).reshape(H, W)
                     for c in range(tgt.shape[2])])
    image = np.clip(sols, 0, 255).astype(tgt.dtype).transpose(1, 2, 0)
    return sols, np.ascontiguousarray(image)


def safe_pixels(sol, guard):
    """Where a truncation of ``sol`` to 8 bits cannot flip within ``guard``: farther than guard
    from every integer of 1..255 that it could cross (values beyond the clip range count as safe
    when farther than guard from 0 or 255)."""
    s = np.asarray(sol, np.float64)
    inside = (s > -guard) & (s < 255 + guard)
    near = np.abs(s - np.rint(s)) <= guard
    return ~(inside & near)


def seam_mask(H, W, seed=0):
    """A seam-like mask: everything right of a wiggling vertical seam near the middle, so it
    covers about half the pixels and touches the top, the bottom and the right edge."""
    rng = np.random.default_rng(seed)
    y = np.arange(H)
    phase = rng.uniform(0, 2 * np.pi, 3)
    seam = W * (0.5 + 0.06 * np.sin(2 * np.pi * y / H * 1.5 + phase[0])
                + 0.03 * np.sin(2 * np.pi * y / H * 5 + phase[1])
                + 0.01 * np.sin(2 * np.pi * y / H * 17 + phase[2]))
    return np.arange(W)[None, :] >= seam[:, None]


def textured(H, W, C, seed):
    """A seeded uint8 test image: smoothed noise plus 8 levels of white noise, so no region is
    flat (a flat region's exact solution is an integer and its truncation a coin toss)."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0, 255, (H, W, C))
    k = np.ones(9) / 9
    for _ in range(3):
        img = np.apply_along_axis(lambda r: np.convolve(np.pad(r, 4, mode="edge"), k, "valid"),
                                  0, img)
        img = np.apply_along_axis(lambda r: np.convolve(np.pad(r, 4, mode="edge"), k, "valid"),
                                  1, img)
    img = (img - img.min()) / (img.max() - img.min()) * 200 + 20
    img = img + rng.uniform(-4, 4, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
