"""NumPy restatement of the median blend's contract on patches of the
blender protocol: ``(warped float32 [h][w][4], mask bool [h][w], irange)``.

Vectorised over the pixels, a loop over the patches.  float32 wherever the contract says
float32, one rounding per operation; the weights are int64, so their sums are exact whatever
order they are taken in."""
import numpy as np

SCALE = np.float32(2.0 ** 30)


def stack(patches, shape):
    """The samples as planes over the mosaic: present bool [n][H][W] (the patch covers the pixel
    and is unmasked there), colour float32 [n][H][W][3], alpha float32 [n][H][W]."""
    H, W = shape
    n = len(patches)
    present = np.zeros((n, H, W), bool)
    colour = np.zeros((n, H, W, 3), np.float32)
    alpha = np.zeros((n, H, W), np.float32)
    for i, (warped, mask, irange) in enumerate(patches):
        present[i][irange] = ~np.asarray(mask).astype(bool)
        colour[i][irange] = np.asarray(warped, np.float32)[..., :3]
        alpha[i][irange] = np.asarray(warped, np.float32)[..., 3]
    return present, colour, alpha


def weights(present, alpha):
    """w_i = trunc(clamp(a_i, 0, 1) 2^30), 0 where there is no sample; int64."""
    w = np.trunc(np.clip(alpha, np.float32(0), np.float32(1)) * SCALE).astype(np.int64)
    return np.where(present, w, 0)


def median_index(present, colour, alpha):
    """(j int [H][W], T int64 [H][W]): the median sample's patch index where T > 0 (else 0)."""
    w = weights(present, alpha)
    total = w.sum(axis=0)
    key = (colour[..., 0] + colour[..., 1]) + colour[..., 2]          # float32, two roundings
    voting = w > 0
    # ascending (key, index) with the non-voting samples last: lexsort is stable, so equal keys
    # stay in index order
    order = np.lexsort((key, ~voting), axis=0)
    run = np.cumsum(np.take_along_axis(w, order, axis=0), axis=0)
    first = np.argmax(2 * run >= total[None], axis=0)
    j = np.take_along_axis(order, first[None], axis=0)[0]
    return np.where(total > 0, j, 0), total


def inliers(present, colour, alpha, tol):
    """bool [n][H][W]: the samples the result is blended over."""
    j, total = median_index(present, colour, alpha)
    cj = np.take_along_axis(colour, j[None, :, :, None], axis=0)[0]   # [H][W][3]
    close = (np.abs(colour - cj[None]) <= np.float32(tol)).all(axis=-1)
    return present & (close | (total == 0)[None])


def blend_over(members, colour, alpha):
    """linear_blend's arithmetic over the chosen samples, in index order -> uint8 [H][W][3]."""
    n, H, W = members.shape
    acc = np.zeros((H, W, 3), np.float32)
    wsum = np.zeros((H, W), np.float32)
    for i in range(n):
        m = members[i]
        acc[m] = acc[m] + colour[i][m] * alpha[i][m][:, None]
        wsum[m] = wsum[m] + alpha[i][m]
    wsum[wsum == 0] = 1
    return (np.float32(255) * (acc / wsum[..., None])).astype(np.int32).astype(np.uint8)


def median_blend(patches, shape, tol):
    """(mosaic uint8 [H][W][3], valid bool [H][W])."""
    present, colour, alpha = stack(patches, shape)
    return blend_over(inliers(present, colour, alpha, tol), colour, alpha), present.any(axis=0)


def sample_counts(patches, shape):
    """Samples per pixel, int [H][W]."""
    return stack(patches, shape)[0].sum(axis=0)
