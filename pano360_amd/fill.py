"""Filling what no frame covers, on the device (``pano_fill_u8``, ``pano_select_u8``,
csrc/fill.hip): a pull-push fill of a mosaic's invalid pixels, the filled colour carried past the
mosaic's rectangle onto the whole sphere, and views composited over that sphere so that their
covered pixels stay exactly what ``view.render_device`` returns.

``fill_device`` fills a uint8 [H][W][3] image where its mask is 0: the valid pixels are averaged
down the chain of ``view.mip_shapes`` until one pixel is left, then every invalid pixel takes the
9 : 3 : 3 : 1 mix of the four nearest pixels of the level above, from the top down.
``sphere_device`` renders the (filled) mosaic as a 2:1 equirectangular image, fills that too and
adds a row beyond each pole: a closed mosaic that covers every direction.  ``render_filled_device``
renders views from the mosaic and from that sphere and keeps the first wherever the mosaic covers
the pixel.  The arithmetic is stated in include/pano360.h and, in float64, in tests/fill_model.py.
The fill works in the equirectangular plane: near a pole it is smooth, not isotropic; and on a
closed image whose width is odd at some level the seam is slightly stretched there.  There is no
CPU fallback.
"""
import math

import numpy as np

from . import _lib
from . import view as _view

TAIL_PIXELS = _lib.FILL_TAIL_PIXELS
TEXEL = 16                          # bytes of a level >= 1's pixel: float32 r, g, b, validity
HEADER = 256                        # the workspace starts with the "any pixel valid" word


# ------------------------------------------------------------------- layout
def level_shapes(h, w):
    """[(H_l, W_l)] of the fill's chain: ``view.mip_shapes``, which ends at 1 x 1 for sides up to
    ``view.MAX_SIDE``."""
    h, w = int(h), int(w)
    if not (1 <= h <= _view.MAX_SIDE and 1 <= w <= _view.MAX_SIDE):
        raise ValueError(f"an image of {h} x {w}: sides 1 .. {_view.MAX_SIDE}")
    return _view.mip_shapes(h, w)


def tail_level(h, w):
    """The first level of at most ``TAIL_PIXELS`` pixels: one workgroup takes it down to 1 x 1 and
    back up; the levels 1 .. tail - 1 are one pull and one push launch each, level 0 one push."""
    return next(l for l, (a, b) in enumerate(level_shapes(h, w)) if a * b <= TAIL_PIXELS)


def level_offsets(h, w):
    """Byte offset of every level >= 1 in the workspace (entry 0 is 0: level 0 is the image; each
    level dense at ``TEXEL`` bytes per pixel, its start on 256 bytes, behind the header) and, last,
    the workspace's size."""
    offs, at = [0], HEADER
    for a, b in level_shapes(h, w)[1:]:
        offs.append(at)
        at = (at + TEXEL * a * b + 255) // 256 * 256
    return offs + [at]


def launches(h, w):
    """(pulls, pushes) launched around the tail's one workgroup."""
    tail = tail_level(h, w)
    return max(tail - 1, 0), tail


# ------------------------------------------------------------------ the fill
def _check_mask(mask, shape):
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"a mask of shape {tuple(mask.shape)} for an image of {tuple(shape)}")
    if str(mask.dtype) not in ("uint8", "bool", "torch.uint8", "torch.bool"):
        raise ValueError(f"a mask of {mask.dtype}: uint8 or bool")


def _device_mask(mask, eng):
    import torch
    if not isinstance(mask, torch.Tensor):
        mask = torch.from_numpy(np.ascontiguousarray(mask))
    mask = mask.to(torch.device(eng.device))
    if mask.stride(1) != 1 or mask.stride(0) < mask.shape[1]:
        mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def fill_device(image, mask, closed=False, eng=None, out=None):
    """The uint8 [H][W][3] ``image`` with the pixels whose ``mask`` (uint8 or bool [H][W]) is 0
    filled from the valid ones; ``closed``: column W is column 0.  Device tensors (crop views need
    no copy as long as a row's pixels are contiguous) or host arrays, which are uploaded.  Returns
    a new device tensor; ``out=image`` (a device tensor) fills in place.  Queued on the engine's
    stream."""
    import torch
    _view._check_mosaic(image)
    _check_mask(mask, image.shape[:2])
    eng = _lib._engine(eng)
    in_place = out is not None and out is image
    image = _lib.rgb_on_device(image, eng)
    if in_place and image is not out:
        raise ValueError("out=image: a device tensor whose rows' pixels are contiguous")
    mask = _device_mask(mask, eng)
    h, w = int(image.shape[0]), int(image.shape[1])
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=image.device)
    elif in_place:
        out = image
    elif tuple(out.shape) != (h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("out: the image itself or a dense uint8 tensor of its shape")
    eng.call("pano_fill_u8", image, image.stride(0), mask, mask.stride(0), h, w, 1 if closed else 0,
             out, out.stride(0))
    return out


def select_device(a, mask, b, eng=None, out=None):
    """``mask ? a : b`` per pixel of two dense uint8 [h][w][3] device tensors (``mask`` uint8
    [h][w]); ``out`` may be ``a`` or ``b``."""
    import torch
    eng = _lib._engine(eng)
    if a.shape != b.shape or tuple(mask.shape) != tuple(a.shape[:2]) or a.shape[-1] != 3:
        raise ValueError(f"images of {tuple(a.shape)} and {tuple(b.shape)}, a mask of {tuple(mask.shape)}")
    if out is None:
        out = torch.empty_like(a)
    for t in (a, mask, b, out):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError("select_device: dense uint8 tensors")
    eng.call("pano_select_u8", a, mask, b, out, mask.numel())
    return out


# --------------------------------------------------------------- the sphere
def sphere_width(geom):
    """The default width of ``sphere_device``: the mosaic's columns per turn, even, at most 4096
    (the background is smooth and need not have the mosaic's resolution)."""
    return max(2, min(4096, 2 * round(math.pi / geom.resolution[0])))


def sphere_geometry(width):
    """The geometry of ``sphere_device``'s image: the 2:1 equirectangular rows of
    ``view.equirect(width)`` and one more beyond each pole; closed.  Every direction, the poles
    included, lies between two of its rows."""
    width = int(width)
    if width < 2 or width % 2:
        raise ValueError(f"width {width}: even, >= 2")
    sa, sb = 2 * math.pi / width, math.pi / (width // 2)
    return _view.MosaicGeometry((-math.pi + sa / 2, -math.pi / 2 - sb / 2), (sa, sb),
                                (width // 2 + 2, width))


def sphere_device(mosaic, geom, valid=None, width=None, eng=None):
    """The whole sphere behind a mosaic: (sphere, its ``view.MosaicGeometry``).  The mosaic is
    filled where ``valid`` (if given) is 0, rendered as ``view.equirect(width)``, and that image is
    filled where the render's mask is 0, as a closed image.  One row is added beyond each pole, the
    neighbouring row rolled by ``width // 2``: the image continued over the pole, so that the
    renderer's row clamp never leaves a hole there.  uint8 [width // 2 + 2][width][3]."""
    import torch
    eng = _lib._engine(eng)
    width = sphere_width(geom) if width is None else int(width)
    sphere_geom = sphere_geometry(width)
    if valid is not None:
        mosaic = fill_device(mosaic, valid, geom.closed, eng)
    images, masks = _view.render_device(mosaic, geom, [_view.equirect(width)], eng)
    rows, half = width // 2, width // 2
    sphere = torch.empty((rows + 2, width, 3), dtype=torch.uint8, device=images[0].device)
    fill_device(images[0], masks[0], True, eng, out=sphere[1:rows + 1])
    for pole, near in ((0, 1), (rows + 1, rows)):
        sphere[pole, half:] = sphere[near, :width - half]
        sphere[pole, :half] = sphere[near, width - half:]
    return sphere, sphere_geom


def render_filled_device(mosaic_or_mips, geom, views, background, eng=None):
    """``view.render_device`` of ``views``, with the pixels the mosaic does not cover taken from
    the same views of ``background`` = (``view.Mips`` or image, geometry) of ``sphere_device``.
    Covered pixels are bit for bit what ``render_device`` returns.  Returns (images, masks), the
    masks as from the mosaic's render."""
    eng = _lib._engine(eng)
    views = list(views)
    back_source, back_geom = background
    images, masks = _view.render_device(mosaic_or_mips, geom, views, eng)
    behind, _ = _view.render_device(back_source, back_geom, views, eng)
    for image, mask, back in zip(images, masks, behind):
        select_device(image, mask, back, eng, out=image)
    return images, masks


# ------------------------------------------------------------- host wrappers
def fill(image, mask, closed=False, eng=None):
    """``fill_device`` on host arrays: the filled image as a NumPy array."""
    return fill_device(np.asarray(image), np.asarray(mask), closed, eng).cpu().numpy()
