"""``blend.laplacian_blending``, ``blend.poisson_blend``, ``blend.graph_cut`` and
``blend.alpha_blend`` of the reference (blend.py:48-203) on the GPU, and the 8-bit shrink the
CLI applies to its inputs (stitcher.py:418-420).

Same call as the reference: ``laplacian_blending(img1, img2, mask=None, n_levels=6)``
with uint8 (or float) ``[H][W][C]`` images and an optional float ``[H][W][1 or C]``
mask; returns uint8 ``[H][W][C]``.  The image pyramids are float32, the mask pyramid
and everything after the per-level mix float64, as NumPy's promotion makes them in the
reference.  ``poisson_blend(img_source, img_target, img_mask)`` writes the seamless clone of
the source into the target at the mask pixels; its sparse systems are solved by a float64
BiCGStab iteration on the device instead of the reference's direct factorisation.
``graph_cut(img1, img2, shrink=5)`` finds the seam of an overlap - the mask both blenders take -
by the reference's two-marker priority flood, restated as a sweep over (level, colour) classes
that gives the heap loop's labels bit for bit (include/pano360.h); ``alpha_blend`` is its
elementwise mix.  ``blend_overlap_device`` chains them as the reference's ``main()`` does.  All
arithmetic runs in ``libpano360_hip.so`` (``pano_pyr_down_image``, ``pano_pyr_up_image``,
``pano_laplacian_mix``, ``pano_clip_u8``, ``pano_poisson_blend``, ``pano_seam_levels``,
``pano_seam_flood``, ``pano_seam_mask``, ``pano_alpha_blend``, ``pano_resize_u8``); there is
no CPU fallback.  Outside the scope stay ``warp`` (its ``cv2.remap`` with
``BORDER_TRANSPARENT`` and no destination leaves every pixel outside the source undefined) and
``poisson_matrix``: it returns a SciPy sparse matrix, the product does not depend on SciPy, and
the device solver applies the same stencil straight from the mask without building a matrix.
"""
import numpy as np

from . import _lib
from . import engine as _eng


def _dtype_name(t):
    return str(t.dtype).replace("torch.", "")


class _Pyr:
    """Pyramid primitives on interleaved device images [h][w][c]."""

    def __init__(self, eng):
        import torch
        self.eng, self.torch = eng, torch

    def _wide(self, img):
        return int(img.dtype == self.torch.float64)

    def down(self, img):
        h, w, c = img.shape
        out = self.torch.empty(((h + 1) // 2, (w + 1) // 2, c), dtype=img.dtype,
                               device=img.device)
        self.eng.call("pano_pyr_down_image", img, h, w, c, self._wide(img), out)
        return out

    def up(self, img, like, mode):
        """pyrUp(img)[:h, :w] with (h, w) = like.shape[:2]; mode 1: like - up, 2: like + up."""
        sh, sw, c = img.shape
        oh, ow = like.shape[:2]
        out = self.torch.empty((oh, ow, c), dtype=img.dtype, device=img.device)
        self.eng.call("pano_pyr_up_image", img, sh, sw, c, self._wide(img), like, mode, out, oh,
                      ow)
        return out

    def reduce_chain(self, img, depth):
        """[img, pyrDown(img), pyrDown^2(img), ...]: depth + 1 images (blend.py:117-122)."""
        chain = [img]
        while len(chain) <= depth:
            chain.append(self.down(chain[-1]))
        return chain

    def detail_chain(self, img, depth):
        """Coarsest image first, then each finer image minus the expanded coarser one
        (blend.py:124-130)."""
        chain = self.reduce_chain(img, depth)
        levels = [chain[depth]]
        for k in range(depth, 0, -1):
            levels.append(self.up(chain[k], chain[k - 1], 1))
        return levels


def _as_f32(eng, img):
    """``img.astype("float32")`` on the device (blend.py:132-133)."""
    import torch
    img = np.ascontiguousarray(img)
    if img.dtype == np.uint8:
        dev = torch.from_numpy(img).to(eng.device)
        out = torch.empty(img.shape, dtype=torch.float32, device=eng.device)
        eng.call("pano_u8_to_f32", dev, img.size, out)
        return out
    return torch.from_numpy(img.astype(np.float32)).to(eng.device)


def default_mask(shape):
    """The mask the reference builds when none is given (blend.py:107-111): a logistic
    step across the width, 1 / (1 + exp(-100 u)) with u falling linearly from 1 at the left
    edge to -1 at the right, the same on every row and channel; float64."""
    rows, cols, chans = shape
    ramp = np.linspace(1, -1, cols)
    step = 1.0 / (1 + np.exp(-100 * ramp))
    return np.broadcast_to(step[None, :, None], (rows, cols, chans)).copy()


def laplacian_blending_device(img1, img2, mask=None, n_levels=6, eng=None):
    """``laplacian_blending`` on device tensors, no host round trip: uint8 or float32
    ``[H][W][C]`` images, ``mask`` a float32 / float64 device tensor ``[H][W][1 or C]`` or None
    (the reference's default); returns the uint8 device image."""
    import torch
    eng = eng or _eng.engine()
    if img1.dim() != 3 or img1.shape != img2.shape or img1.shape[2] > 4:
        raise ValueError("laplacian_blending: two H x W x C images of one shape, C <= 4")
    rows, cols, chans = img1.shape
    if mask is None:
        # the default mask is one row of float64 repeated: only that row crosses the bus (as
        # a 200 MB host array it was 28 of a 4K blend's 32 ms)
        mask = torch.from_numpy(default_mask((1, cols, 1))).to(eng.device)
        mask = mask.expand(rows, cols, chans)
    elif mask.shape[2] == 1:                       # blend.py:113-114
        mask = mask.expand(rows, cols, chans)
    if not mask.dtype.is_floating_point:
        raise NotImplementedError("integer masks take OpenCV's fixed-point pyramids, "
                                  "which this build does not restate")
    smallest = min(rows, cols) >> (n_levels - 1) if n_levels else 2
    if smallest < 2:
        raise ValueError(f"n_levels={n_levels} leaves a pyramid level narrower than 2 pixels")
    wide = mask.dtype != torch.float32             # float16 / float64 -> float64 like NumPy's mix
    tdtype = torch.float64 if wide else torch.float32
    dev_mask = mask.to(tdtype).contiguous()
    pyr = _Pyr(eng)
    details1 = pyr.detail_chain(_dev_f32(eng, img1), n_levels)
    details2 = pyr.detail_chain(_dev_f32(eng, img2), n_levels)
    weights = pyr.reduce_chain(dev_mask, n_levels)
    blended = None
    # coarsest level first; the weight pyramid is walked from its coarsest end (blend.py:134-138)
    for first, second, weight in zip(details1, details2, reversed(weights)):
        mixed = torch.empty(first.shape, dtype=tdtype, device=eng.device)
        eng.call("pano_laplacian_mix", first, second, weight, first.numel(), int(wide), mixed)
        blended = mixed if blended is None else pyr.up(blended, mixed, 2)
    out = torch.empty(blended.shape, dtype=torch.uint8, device=eng.device)
    eng.call("pano_clip_u8", blended, blended.numel(), int(wide), out)
    return out


def _dev_f32(eng, img):
    """``img.astype("float32")`` of a device image (blend.py:132-133)."""
    import torch
    img = img.contiguous()
    if img.dtype == torch.uint8:
        out = torch.empty(img.shape, dtype=torch.float32, device=eng.device)
        eng.call("pano_u8_to_f32", img, img.numel(), out)
        return out
    return img.to(torch.float32)


def laplacian_blending(img1, img2, mask=None, n_levels=6):
    """Use a Laplacian pyramid on the images for blending (blend.py:105-140).

    Same call and result type as the reference.  The mask keeps its float type the way
    NumPy's promotion keeps it there: float64 (the default mask) makes the per-level mix
    and the collapse float64, a float32 mask keeps them float32.  Limit: every pyramid
    level must be at least 2 pixels wide and high (OpenCV's pyrUp of a 1-pixel row is not
    restated here); integer masks are not supported."""
    import torch
    eng = _eng.engine()
    if img1.ndim != 3 or img1.shape != img2.shape or img1.shape[2] > 4:
        raise ValueError("laplacian_blending: two H x W x C images of one shape, C <= 4")
    if mask is not None:
        if not np.issubdtype(mask.dtype, np.floating):
            raise NotImplementedError("integer masks take OpenCV's fixed-point pyramids, "
                                      "which this build does not restate")
        mdtype = np.float32 if mask.dtype == np.float32 else np.float64
        mask = torch.from_numpy(np.ascontiguousarray(mask, dtype=mdtype)).to(eng.device)
    return laplacian_blending_device(_as_f32(eng, img1), _as_f32(eng, img2), mask, n_levels,
                                     eng).cpu().numpy()


# ---------------------------------------------------------------- Poisson blend
# ||r||_2 <= POISSON_RTOL ||b||_2 stops a channel.  What matters is the solution's error against
# the reference's direct solve, which the result's truncation to 8 bits makes visible: the tests
# hold it to 1e-4 of a grey level.  For the reference's matrix the error a residual leaves grows
# with the mask's extent; the same recurrence run in NumPy against SciPy's direct solve, on
# half-plane masks, left at most 1.6e-5 (300 x 260) and 5.4e-5 (540 x 488) at 1e-10, and
# 3.6e-8 / 3.8e-7 at 1e-12, for 20 % more iterations.  1e-12 keeps a factor of 250 at 540 x 488
# and is still a hundred times above where float64 stalls (below 1e-13 the recurrence's
# residual and the true one part).
POISSON_RTOL = 1e-12
# Iterations grow about linearly with the mask's width (230 at 128 columns, 930 at 488); an
# overlap of a thousand columns needs about two thousand.  The cap is there to end a solve that
# stalls, not to bound a healthy one.
POISSON_MAX_ITERS = 20000


def poisson_blend_device(src, tgt, mask, eng=None, want_solution=False,
                         max_iters=POISSON_MAX_ITERS):
    """``poisson_blend`` on device tensors, no host round trip: src, tgt uint8 ``[H][W][C]``
    (C <= 4, contiguous), mask ``[H][W]`` of any dtype (``!= 0`` selects).  ``tgt`` is written
    in place at the mask pixels and returned.  With ``want_solution`` returns
    ``(tgt, solution, iters, resid)``: the float64 solution ``[C][H][W]`` (device), and per
    channel the iterations used and the final ``||r|| / ||b||`` (host arrays).  Raises
    ``PanoError`` when a channel reaches ``max_iters`` or BiCGStab breaks down; ``tgt`` is then
    untouched: an unconverged image is never returned."""
    import torch
    eng = eng or _eng.engine()
    if src.dim() != 3 or src.shape != tgt.shape or not 1 <= src.shape[2] <= 4:
        raise ValueError("poisson_blend: two H x W x C images of one shape, C <= 4")
    if src.dtype != torch.uint8 or tgt.dtype != torch.uint8:
        raise NotImplementedError("poisson_blend: uint8 images only (the reference's result for "
                                  "other types is not restated)")
    h, w, c = src.shape
    if tuple(mask.shape) != (h, w):
        raise ValueError(f"poisson_blend: the mask is {tuple(mask.shape)}, the images {h} x {w}")
    if w < 2:
        raise ValueError("poisson_blend: images narrower than 2 pixels (the reference's own "
                         "matrix cannot be built for them)")
    if not tgt.is_contiguous():
        raise ValueError("poisson_blend: the target must be contiguous (it is written in place)")
    src = src.contiguous()
    sel = (mask != 0).to(torch.uint8).contiguous()
    iters = np.zeros(c, np.int32)
    resid = np.zeros(c, np.float64)
    solution = None
    if bool(sel.any()):
        if want_solution:
            solution = torch.empty((c, h, w), dtype=torch.float64, device=tgt.device)
        eng.call("pano_poisson_blend", src, tgt, sel, h, w, c, POISSON_RTOL, int(max_iters),
                 solution, iters, resid)
    elif want_solution:                            # an empty mask: the solution is the target
        solution = tgt.permute(2, 0, 1).to(torch.float64).contiguous()
    return (tgt, solution, iters, resid) if want_solution else tgt


def poisson_blend(img_source, img_target, img_mask):
    """Combine images using Poisson editing (blend.py:175-203).

    Same call as the reference: two uint8 ``H x W x C`` images of one shape (C <= 4) and a mask
    ``H x W`` of any dtype whose nonzero pixels are solved for.  The result is written into
    ``img_target`` and that array is returned; per channel it is ``np.clip(sol, 0, 255)``
    truncated to uint8, with ``sol`` the solution of the reference's own linear system (its
    border quirks included, include/pano360.h) to well within 1e-4 of a grey level.  Images
    of another dtype raise ``NotImplementedError``.  ``poisson_matrix`` is not provided: it
    returns a SciPy sparse matrix and the product does not depend on SciPy."""
    import torch
    eng = _eng.engine()
    for img in (img_source, img_target):
        if not isinstance(img, np.ndarray) or img.ndim != 3:
            raise ValueError("poisson_blend: two H x W x C NumPy images of one shape, C <= 4")
        if img.dtype != np.uint8:
            raise NotImplementedError("poisson_blend: uint8 images only (the reference's result "
                                      "for other types is not restated)")
    sel = np.asarray(img_mask) != 0
    out = poisson_blend_device(torch.from_numpy(np.ascontiguousarray(img_source)).to(eng.device),
                               torch.from_numpy(np.ascontiguousarray(img_target)).to(eng.device),
                               torch.from_numpy(sel).to(eng.device), eng)
    if sel.any():
        img_target[...] = out.cpu().numpy()
    return img_target


# ---------------------------------------------------------------- seam (graph_cut, alpha_blend)
_SEAM_TYPES = tuple(_lib.SEAM_DTYPES)


def seam_border(shrink):
    """Columns of each preset band of the seam's grid (blend.py:74)."""
    return int(13 / shrink) + 1


def _seam_check(shape1, shape2, dtype1, dtype2, shrink):
    """The input domain of ``graph_cut`` that shapes and types decide; returns (rows, cols,
    border) of the grid."""
    if len(shape1) != 3 or tuple(shape1) != tuple(shape2) or not 1 <= shape1[2] <= 4:
        raise ValueError("graph_cut: two H x W x C images of one shape, 1 <= C <= 4")
    if dtype1 != dtype2 or dtype1 not in _SEAM_TYPES:
        raise NotImplementedError(f"graph_cut: images of {dtype1} / {dtype2} are not restated "
                                  f"(one of {', '.join(_SEAM_TYPES)} for both)")
    if int(shrink) != shrink or shrink < 1:
        raise ValueError(f"graph_cut: shrink={shrink!r} must be an integer >= 1")
    if dtype1 == "uint8" and shape1[2] == 4:
        raise OverflowError("graph_cut: uint8 images with an alpha channel: the reference cannot "
                            "store its -1 in a uint8 difference (pass img.astype(np.int16))")
    rows, cols, border = shape1[0] // shrink, shape1[1] // shrink, seam_border(shrink)
    if rows < 1 or cols < 2 * border + 1:
        raise ValueError(f"graph_cut: a {rows} x {cols} grid is too small for preset bands of "
                         f"{border} columns (shrink={shrink})")
    return rows, cols, border


def _float_taps(n_out, n_in):
    """(first tap, second tap, bits of the float32 weights 1 - f and f) per output sample of
    cv2.resize's float INTER_LINEAR pass; the coordinate is formed as ``_resize_taps`` forms it,
    from the scale ``1 / (n_out / n_in)`` OpenCV derives from an explicit ``dsize``."""
    scale = 1.0 / (float(n_out) / float(n_in))
    f = ((np.arange(n_out) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    f[s < 0] = 0
    s[s < 0] = 0
    f[s >= n_in - 1] = 0
    s[s >= n_in - 1] = n_in - 1
    tab = np.empty((n_out, 4), np.int32)
    tab[:, 0], tab[:, 1] = s, np.minimum(s + 1, n_in - 1)
    tab[:, 2] = (np.float32(1.0) - f).view(np.int32)
    tab[:, 3] = f.view(np.int32)
    return tab


def seam_levels_device(img1, img2, shrink, eng):
    """The flood's priorities, int16 ``[H // shrink][W // shrink]`` (``pano_seam_levels``), and
    the device word that is 1 when a value was outside the integers 0..255."""
    import torch
    h, w, c = img1.shape
    level = torch.empty((h // shrink, w // shrink), dtype=torch.int16, device=img1.device)
    bad = torch.empty(1, dtype=torch.int32, device=img1.device)
    code = _lib.SEAM_DTYPES[_dtype_name(img1)]
    eng.call("pano_seam_levels", img1, img2, code, h, w, c, int(shrink), level, bad)
    return level, bad


def seam_flood_device(level, border, eng, path=0, want_stats=False):
    """int8 labels of a level grid (``pano_seam_flood``); with ``want_stats`` also the device
    int32 ``[4]`` the call fills (include/pano360.h)."""
    import torch
    rows, cols = level.shape
    labels = torch.empty((rows, cols), dtype=torch.int8, device=level.device)
    stats = torch.zeros(4, dtype=torch.int32, device=level.device) if want_stats else None
    eng.call("pano_seam_flood", level, rows, cols, border, int(path), labels, stats)
    return (labels, stats) if want_stats else labels


def seam_mask_device(labels, h, w, eng):
    """blend.py:99-100 on the device: uint8 ``[h][w][1]`` (``pano_seam_mask``)."""
    import torch
    rows, cols = labels.shape
    xtab = eng.to_device(_float_taps(w, cols))
    ytab = eng.to_device(_float_taps(h, rows))
    mask = torch.empty((h, w, 1), dtype=torch.uint8, device=labels.device)
    eng.call("pano_seam_mask", labels, rows, cols, xtab, ytab, mask, h, w)
    return mask


def graph_cut_device(img1, img2, shrink=5, eng=None, want_labels=False, path=0):
    """``graph_cut`` on device tensors, no host round trip of the images or the mask: two
    contiguous ``[H][W][C]`` tensors in (the domain of ``graph_cut``), the uint8 mask
    ``[H][W][1]`` on the device out - what ``poisson_blend_device`` takes as ``mask[..., 0] >
    127``.  With ``want_labels`` returns ``(mask, labels)``, the int8 label grid ``[H // shrink]
    [W // shrink]`` (-1 / +1; 0 never survives the flood).  ``path`` forces the flood's kernel:
    0 by size, 1 one workgroup with the grid in LDS, 2 tiles (``pano_seam_flood``).  One word is
    read back (the domain check), so the call waits for the stream."""
    import torch
    eng = eng or _eng.engine()
    name = _dtype_name(img1)
    rows, cols, border = _seam_check(img1.shape, img2.shape, name, _dtype_name(img2), shrink)
    shrink = int(shrink)
    h, w = img1.shape[:2]
    img1, img2 = img1.contiguous(), img2.contiguous()
    level, bad = seam_levels_device(img1, img2, shrink, eng)
    if border == 1:
        # blend.py:75-76: the +1 band's slice is [:, 0:], every cell is preset and nothing floods
        labels = torch.ones((rows, cols), dtype=torch.int8, device=img1.device)
    else:
        labels = seam_flood_device(level, border, eng, path)
    mask = seam_mask_device(labels, h, w, eng)
    if int(bad.item()):
        raise NotImplementedError("graph_cut: the images hold values other than the integers "
                                  "0..255 (real-valued differences are not restated)")
    return (mask, labels) if want_labels else mask


def graph_cut(img1, img2, shrink=5):
    """The seam between two images of an overlap (blend.py:56-100); despite the name a
    two-marker priority flood, not a min-cut.

    Same call and result as the reference: two host images of one shape ``[H][W][C]``, the
    uint8 mask ``[H][W][1]`` out, 255 where ``img1`` owns the pixel, 0 where ``img2`` does,
    bilinear in between at the seam.  Input domain (checked; everything else raises before the
    device is touched):

    * ``C`` in 1..4 and **integers 0..255** as int16, int32, float32 or float64; with four
      channels a pixel whose fourth is 0 in either image gets the lowest priority (-1).  Other
      values raise ``NotImplementedError``: real-valued differences are not restated.
    * uint8 images are taken as the reference takes them: it subtracts and negates in uint8, so
      its differences wrap (``3 - 5 = 254``) and its priorities run 0, 255, 254, .. 1; the same
      seam comes out here.  uint8 with four channels raises ``OverflowError`` as the reference
      does under NumPy 2.  A caller who wants true differences passes ``img.astype(np.int16)``.
    * ``shrink`` an integer >= 1; ``shrink >= 14`` gives the reference's all-(+1) grid, an
      all-zero mask.  A grid ``[H // shrink][W // shrink]`` with fewer than
      ``2 * (int(13 / shrink) + 1) + 1`` columns or no rows raises ``ValueError``."""
    import torch
    img1, img2 = np.asarray(img1), np.asarray(img2)
    _seam_check(img1.shape, img2.shape, img1.dtype.name, img2.dtype.name, shrink)
    if img1.dtype != np.uint8:
        for img in (img1, img2):
            if not (np.isfinite(img).all() and img.min() >= 0 and img.max() <= 255
                    and np.array_equal(img, np.rint(img))):
                raise NotImplementedError("graph_cut: the images hold values other than the "
                                          "integers 0..255 (real-valued differences are not "
                                          "restated)")
    eng = _eng.engine()
    mask = graph_cut_device(torch.from_numpy(np.ascontiguousarray(img1)).to(eng.device),
                            torch.from_numpy(np.ascontiguousarray(img2)).to(eng.device),
                            shrink, eng)
    return mask.cpu().numpy()


def alpha_blend_device(img1, img2, mask=None, eng=None):
    """``alpha_blend`` on device tensors: images ``[H][W][C]`` of one dtype (uint8, int16, int32,
    float32, float64), ``mask`` a float32 / float64 tensor broadcastable to them (``[1][W][1]``,
    ``[H][W][1]``, ``[H][W][C]``) or None for the reference's ramp; uint8 ``[H][W][C]`` out."""
    import torch
    eng = eng or _eng.engine()
    if img1.dim() != 3 or img1.shape != img2.shape or img1.dtype != img2.dtype:
        raise ValueError("alpha_blend: two H x W x C images of one shape and dtype")
    name = _dtype_name(img1)
    if name not in _SEAM_TYPES:
        raise NotImplementedError(f"alpha_blend: images of {name}")
    h, w, c = img1.shape
    if mask is None:
        mask = torch.from_numpy(np.linspace(1, 0, w).reshape((1, w, 1))).to(eng.device)
    if mask.dtype not in (torch.float32, torch.float64):
        raise NotImplementedError(f"alpha_blend: a mask of {mask.dtype}")
    if mask.dim() != 3 or any(m not in (1, n) for m, n in zip(mask.shape, img1.shape)):
        raise ValueError(f"alpha_blend: a mask of {tuple(mask.shape)} does not broadcast to "
                         f"{tuple(img1.shape)}")
    mask = mask.contiguous()
    strides = [0 if m == 1 else st for m, st in zip(mask.shape, mask.stride())]
    out = torch.empty((h, w, c), dtype=torch.uint8, device=img1.device)
    eng.call("pano_alpha_blend", img1.contiguous(), img2.contiguous(), _lib.SEAM_DTYPES[name], mask,
             int(mask.dtype == torch.float64), *strides, h, w, c, out)
    return out


def alpha_blend(img1, img2, mask=None):
    """Blend using an alpha ramp (blend.py:48-53): ``(img1*mask + img2*(1-mask))`` truncated to
    uint8, the two products and the sum rounded separately in NumPy's promoted type (float64;
    float32 for a float32 mask with uint8, int16 or float32 images), so the bytes are NumPy's.
    The default mask is the reference's ``linspace(1, 0, W)`` ramp."""
    import torch
    img1, img2 = np.asarray(img1), np.asarray(img2)
    if img1.ndim != 3 or img1.shape != img2.shape or img1.dtype != img2.dtype:
        raise ValueError("alpha_blend: two H x W x C images of one shape and dtype")
    if mask is not None:
        mask = np.asarray(mask)
        if mask.dtype not in (np.float32, np.float64):
            raise NotImplementedError(f"alpha_blend: a mask of {mask.dtype}")
    eng = _eng.engine()
    dev = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(eng.device)
    return alpha_blend_device(torch.from_numpy(np.ascontiguousarray(img1)).to(eng.device),
                              torch.from_numpy(np.ascontiguousarray(img2)).to(eng.device), dev,
                              eng).cpu().numpy()


def blend_overlap_device(img1, img2, delta, blender="poisson", shrink=5, eng=None):
    """The body of the reference's ``main()`` (blend.py:219-226) on uint8 device images
    ``[H][W][C]``: the seam of ``img1[:, -delta:]`` / ``img2[:, :delta]`` (as int16, so the
    differences are true ones), the chosen blend of the overlap under it - ``"poisson"``:
    ``poisson_blend_device`` with ``mask > 127``; ``"laplacian"``: the Laplacian blend with
    ``mask / 255.0``; ``"alpha"``: ``alpha_blend`` with ``mask / 255.0`` - and
    ``[img1[:, :-delta], overlap, img2[:, delta:]]`` side by side.  The inputs are not written."""
    import torch
    eng = eng or _eng.engine()
    if blender not in ("poisson", "laplacian", "alpha"):
        raise ValueError(f"blend_overlap_device: blender {blender!r}")
    if img1.dtype != torch.uint8 or img2.dtype != torch.uint8 or img1.shape != img2.shape:
        raise ValueError("blend_overlap_device: two uint8 H x W x C images of one shape")
    if not 0 < delta <= img1.shape[1]:
        raise ValueError(f"blend_overlap_device: delta={delta} of {img1.shape[1]} columns")
    left, right = img1[:, -delta:].contiguous(), img2[:, :delta].contiguous()
    mask = graph_cut_device(left.to(torch.int16), right.to(torch.int16), shrink, eng)
    if blender == "poisson":
        overlap = poisson_blend_device(left, right.clone(), mask[..., 0] > 127, eng)
    elif blender == "laplacian":
        overlap = laplacian_blending_device(left, right, mask.to(torch.float64) / 255.0, 6, eng)
    else:
        overlap = alpha_blend_device(left, right, mask.to(torch.float64) / 255.0, eng)
    return torch.cat([img1[:, :-delta], overlap, img2[:, delta:]], dim=1)


# ---------------------------------------------------------------- CLI ingest
def _resize_taps(n_out, n_in, scale):
    """(first tap, second tap, 11-bit coefficient of each) per output sample of
    cv2.resize's 8-bit INTER_LINEAR path; float32 coordinates as OpenCV keeps them."""
    f = ((np.arange(n_out) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    f[s < 0] = 0
    s[s < 0] = 0
    f[s >= n_in - 1] = 0
    s[s >= n_in - 1] = n_in - 1
    c0 = np.rint((np.float32(1.0) - f) * np.float32(2048.0))
    c1 = np.rint(f * np.float32(2048.0))
    return np.stack([s, np.minimum(s + 1, n_in - 1), c0, c1], axis=1).astype(np.int32)


def shrink_device(frame, shrink, eng=None):
    """``cv2.resize(im, None, fx=1/shrink, fy=1/shrink)`` (stitcher.py:419-420) of a
    uint8 device image [h][w][c]; returns the shrunk device image."""
    import torch
    eng = eng or _eng.engine()
    h, w, c = frame.shape
    fx = 1 / shrink
    ow, oh = int(np.rint(w * fx)), int(np.rint(h * fx))
    if ow < 1 or oh < 1:
        raise ValueError(f"shrink {shrink} leaves nothing of a {w}x{h} image")
    out = torch.empty((oh, ow, c), dtype=torch.uint8, device=frame.device)
    scale = 1.0 / fx
    if abs(scale - 2.0) < np.finfo(float).eps and w % 2 == 0 and h % 2 == 0:
        xtab = ytab = None                         # exact 2:1: the area path
    else:
        xtab = eng.to_device(_resize_taps(ow, w, scale))
        ytab = eng.to_device(_resize_taps(oh, h, scale))
    eng.call("pano_resize_u8", frame, h, w, c, xtab, ytab, out, oh, ow)
    return out


def shrink_images(imgs, shrink):
    """The resize step of the CLI (stitcher.py:418-420): host uint8 images in, shrunk
    uint8 frames resident on the device out (what ``Engine.stitch`` consumes)."""
    import torch
    eng = _eng.engine()
    frames = [torch.from_numpy(np.ascontiguousarray(im)).to(eng.device) for im in imgs]
    if shrink > 1:
        frames = [shrink_device(f, shrink, eng) for f in frames]
    return frames
