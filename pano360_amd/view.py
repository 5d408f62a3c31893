"""Views of a finished mosaic, rendered on the device (``pano_mip_u8``, ``pano_view_render``,
csrc/view.hip): rectilinear looks, cube faces, a full-sphere 2:1 equirectangular image, a little
planet.  What the reference does with ``cv2.imshow("Mosaic", mosaic)`` and a person's eyes.

A mosaic samples the sphere at theta = low[0] + x res[0], phi = low[1] + y res[1]
(``MosaicGeometry``, the values of ``engine.Plan``); the frame is x right, y down, z forward.
``mip_device`` builds the mosaic's mip chain once, ``render_device`` renders any number of views of
it in one launch, each a uint8 [h][w][3] image (the mosaic's channel order) and a uint8 [h][w]
coverage mask.  The arithmetic is stated in include/pano360.h and, in float64, in
tests/view_model.py.  There is no CPU fallback.
"""
import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import _lib

RECTILINEAR, EQUIRECT, STEREOGRAPHIC = (_lib.VIEW_RECTILINEAR, _lib.VIEW_EQUIRECT,
                                        _lib.VIEW_STEREOGRAPHIC)
MAX_LEVELS = _lib.VIEW_MAX_LEVELS
MAX_VIEWS = _lib.VIEW_MAX_VIEWS
MAX_SIDE = _lib.VIEW_MAX_SIDE       # of a view and of a mosaic (pano_view_render's limit)
CUBE_FACES = ("front", "right", "back", "left", "up", "down")
# (right, down) of the faces in that order; forward = right x down: +z, +x, -z, -x, -y, +y
_FACE_AXES = (((1, 0, 0), (0, 1, 0)), ((0, 0, -1), (0, 1, 0)), ((-1, 0, 0), (0, 1, 0)),
              ((0, 0, 1), (0, 1, 0)), ((1, 0, 0), (0, 0, 1)), ((1, 0, 0), (0, 0, -1)))


# ------------------------------------------------------------------ geometry
@dataclass(frozen=True)
class MosaicGeometry:
    """Where a mosaic's pixels lie on the sphere: ``low`` = (theta, phi) of pixel (0, 0),
    ``resolution`` = rad/px along x and y, ``shape`` = (H, W).  ``is_crop``: a rectangle cut out of
    a mosaic, which is never closed."""
    low: tuple
    resolution: tuple
    shape: tuple
    is_crop: bool = False

    def __post_init__(self):
        low = tuple(float(v) for v in self.low)
        res = tuple(float(v) for v in self.resolution)
        shape = tuple(int(v) for v in self.shape)
        if len(low) != 2 or len(res) != 2 or len(shape) != 2:
            raise ValueError("low = (theta, phi), resolution = (x, y), shape = (H, W)")
        if not all(math.isfinite(v) for v in low + res) or min(res) <= 0:
            raise ValueError(f"low {low}, resolution {res}: finite, resolution > 0")
        if min(shape) < 1 or max(shape) > MAX_SIDE:
            raise ValueError(f"shape {shape}: sides 1 .. {MAX_SIDE}")
        if shape[1] * res[0] > 2 * math.pi + res[0] / 2:
            raise ValueError(f"{shape[1]} columns of {res[0]} rad: more than one turn")
        object.__setattr__(self, "low", low)
        object.__setattr__(self, "resolution", res)
        object.__setattr__(self, "shape", shape)

    @property
    def closed(self):
        """The columns go once round the sphere: |W res[0] - 2 pi| < res[0] / 2 (a ring whose
        frames straddle +-pi).  Column W is then column 0."""
        res0 = self.resolution[0]
        return not self.is_crop and abs(self.shape[1] * res0 - 2 * math.pi) < res0 / 2

    def cropped(self, rect):
        """The geometry of the rectangle (y0, x0, h, w) of this mosaic (``crop_mosaic``)."""
        y0, x0, h, w = (int(v) for v in rect)
        if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > self.shape[0] or x0 + w > self.shape[1]:
            raise ValueError(f"rectangle {rect} outside a mosaic of shape {self.shape}")
        return MosaicGeometry((self.low[0] + x0 * self.resolution[0],
                               self.low[1] + y0 * self.resolution[1]),
                              self.resolution, (h, w), True)

    def own_view(self, shift=0):
        """The ``EQUIRECT`` view that samples this mosaic at its own pixels, ``shift`` columns
        further on: on a closed mosaic it renders ``np.roll(mosaic, -shift, axis=1)``."""
        h, w = self.shape
        return equirect_window(self.low[0] + shift * self.resolution[0], self.resolution[0],
                               self.low[1], self.resolution[1], (w, h))

    @classmethod
    def of_plan(cls, plan):
        """The geometry of the mosaic an ``engine.Plan`` describes."""
        return cls(tuple(plan.low), tuple(plan.resolution), tuple(plan.shape))


# --------------------------------------------------------------------- views
@dataclass(frozen=True)
class View:
    """One output image: ``kind``, size ``w`` x ``h``, ``mat`` (float64 3 x 3: M = R K^-1 for
    RECTILINEAR, else R) and four ``params`` (EQUIRECT: a0, sa, b0, sb; STEREOGRAPHIC: cx, cy, f)."""
    kind: int
    w: int
    h: int
    mat: np.ndarray = field(compare=False)
    params: tuple = (0.0, 0.0, 0.0, 0.0)

    def __post_init__(self):
        if self.kind not in (RECTILINEAR, EQUIRECT, STEREOGRAPHIC):
            raise ValueError(f"kind {self.kind}")
        if not (1 <= int(self.w) <= MAX_SIDE and 1 <= int(self.h) <= MAX_SIDE):
            raise ValueError(f"a view of {self.w} x {self.h}: sides 1 .. {MAX_SIDE}")
        mat = np.array(self.mat, np.float64)
        if mat.shape != (3, 3) or not np.isfinite(mat).all() or len(self.params) != 4 \
                or not all(math.isfinite(float(p)) for p in self.params):
            raise ValueError("mat: a finite 3 x 3 matrix, params: four finite values")
        object.__setattr__(self, "mat", mat)
        object.__setattr__(self, "w", int(self.w))
        object.__setattr__(self, "h", int(self.h))
        object.__setattr__(self, "params", tuple(float(p) for p in self.params))


def _size(size):
    w, h = (size, size) if np.isscalar(size) else size
    if int(w) != w or int(h) != h or int(w) < 1 or int(h) < 1:
        raise ValueError(f"size {size!r}: whole numbers >= 1")
    return int(w), int(h)


def rotation(yaw=0.0, pitch=0.0, roll=0.0):
    """R = R_yaw R_pitch R_roll, camera -> mosaic frame: yaw turns right (about y), pitch looks up
    (y is down: the forward axis goes to (0, -sin pitch, cos pitch)), roll turns about the axis."""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    cr, sr = math.cos(roll), math.sin(roll)
    r_yaw = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    r_pitch = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    r_roll = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return r_yaw @ r_pitch @ r_roll


def _rectilinear(rot, f, w, h):
    kinv = np.array([[1 / f, 0, -(w - 1) / (2 * f)], [0, 1 / f, -(h - 1) / (2 * f)], [0, 0, 1.0]])
    return View(RECTILINEAR, w, h, np.asarray(rot, np.float64) @ kinv)


def perspective(yaw, pitch, roll, fov, size):
    """A pinhole look (radians): ``fov`` is the horizontal field of view, in (0, pi); ``size`` =
    (w, h) or one side.  The principal point is the image's centre ((w - 1) / 2, (h - 1) / 2)."""
    w, h = _size(size)
    if not 0 < fov < math.pi:
        raise ValueError(f"fov {fov}: in (0, pi)")
    return _rectilinear(rotation(yaw, pitch, roll), w / (2 * math.tan(fov / 2)), w, h)


def equirect_window(a0, sa, b0, sb, size, rot=None):
    """The ``EQUIRECT`` view theta' = a0 + u sa, phi' = b0 + v sb of ``size`` = (w, h)."""
    w, h = _size(size)
    return View(EQUIRECT, w, h, np.eye(3) if rot is None else rot, (a0, sa, b0, sb))


def equirect(width, yaw=0.0, pitch=0.0, roll=0.0):
    """The full sphere, ``width`` x ``width // 2`` (what a 360 player takes); width even."""
    w, _ = _size(width)
    if w < 2 or w % 2:
        raise ValueError(f"width {width}: even, >= 2")
    sa, sb = 2 * math.pi / w, math.pi / (w // 2)
    return equirect_window(-math.pi + sa / 2, sa, -math.pi / 2 + sb / 2, sb, (w, w // 2),
                           rotation(yaw, pitch, roll))


def face_rotation(face):
    """R of a cube face (index or name of ``CUBE_FACES``): columns right, down, forward."""
    k = CUBE_FACES.index(face) if isinstance(face, str) else int(face)
    right, down = (np.array(a, np.float64) for a in _FACE_AXES[k])
    return np.stack([right, down, np.cross(right, down)], axis=1)


def cube_faces(side):
    """Six ``perspective`` views of ``side`` x ``side`` with f = side / 2, in the order of
    ``CUBE_FACES``: front +z, right +x, back -z, left -x, up -y, down +y."""
    w, h = _size(side)
    return [_rectilinear(face_rotation(k), w / 2, w, h) for k in range(6)]


def little_planet(size, fov=1.5 * math.pi):
    """The stereographic view from above, looking down (+y) at the image's centre: ``fov`` is the
    angle the image's width spans, in (0, 2 pi) (pi: out to the horizon)."""
    w, h = _size(size)
    if not 0 < fov < 2 * math.pi:
        raise ValueError(f"fov {fov}: in (0, 2 pi)")
    f = w / (4 * math.tan(fov / 4))
    return View(STEREOGRAPHIC, w, h, face_rotation("down"), ((w - 1) / 2, (h - 1) / 2, f, 0.0))


# ----------------------------------------------------------------- mip chain
def mip_shapes(h, w):
    """[(H_l, W_l)] of the chain of an H x W image: halved, rounded up, down to 1 x 1 or
    ``MAX_LEVELS`` levels."""
    shapes = [(int(h), int(w))]
    while len(shapes) < MAX_LEVELS and shapes[-1] != (1, 1):
        a, b = shapes[-1]
        shapes.append(((a + 1) // 2, (b + 1) // 2))
    return shapes


def mip_offsets(h, w):
    """Byte offset of every level in the chain's buffer (each level dense, its start rounded up
    to 256 bytes) and, last, the buffer's size."""
    offs = [0]
    for a, b in mip_shapes(h, w):
        offs.append((offs[-1] + 3 * a * b + 255) // 256 * 256)
    return offs


class Mips:
    """A mosaic's mip chain on the device: ``buffer`` (uint8), ``offsets`` (``mip_offsets``),
    ``shape`` = (H, W) of level 0.  ``level(l)`` is a view of level l."""

    def __init__(self, buffer, offsets, shape):
        self.buffer, self.offsets, self.shape = buffer, list(offsets), tuple(shape)

    @property
    def n_levels(self):
        return len(self.offsets) - 1

    def level(self, l):
        h, w = mip_shapes(*self.shape)[l]
        return self.buffer[self.offsets[l]:self.offsets[l] + 3 * h * w].view(h, w, 3)


def _check_mosaic(img):
    shape = tuple(img.shape)
    if not _lib.is_u8(img):
        raise ValueError(f"a mosaic of {img.dtype}: uint8")
    if not _lib.is_rgb_u8(img):
        raise ValueError(f"a mosaic of shape {shape}: [H][W][3]")
    if not (1 <= shape[0] <= MAX_SIDE and 1 <= shape[1] <= MAX_SIDE):
        raise ValueError(f"a mosaic of shape {shape}: sides 1 .. {MAX_SIDE}")


def mip_device(mosaic, eng=None):
    """The mip chain (``Mips``) of a uint8 [H][W][3] mosaic: a device tensor (a crop view needs no
    copy as long as a row's pixels are contiguous) or a host array, which is uploaded.  Queued on
    the engine's stream."""
    import torch
    _check_mosaic(mosaic)
    eng = _lib._engine(eng)
    mosaic = _lib.rgb_on_device(mosaic, eng)
    h, w = int(mosaic.shape[0]), int(mosaic.shape[1])
    offs = mip_offsets(h, w)
    buf = torch.empty(offs[-1], dtype=torch.uint8, device=mosaic.device)
    table = (C.c_int64 * len(offs))(*offs)
    eng.call("pano_mip_u8", mosaic, h, w, mosaic.stride(0), buf, table, len(offs) - 1)
    return Mips(buf, offs, (h, w))


# ------------------------------------------------------------------ renderer
def view_records(views, geom, mips_shape):
    """The ``pano_view`` table of a batch and the ``pano_view_mosaic`` record, as ctypes values
    (output pointers still null).  Checks everything the call would refuse."""
    views = list(views)
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError(f"{len(views)} views: 1 .. {MAX_VIEWS} per call")
    if not isinstance(geom, MosaicGeometry) or tuple(geom.shape) != tuple(mips_shape):
        raise ValueError(f"geometry {getattr(geom, 'shape', geom)!r} for a mosaic of {mips_shape}")
    table = (_lib.View * len(views))()
    for rec, v in zip(table, views):
        if not isinstance(v, View):
            raise ValueError(f"{v!r}: not a view.View")
        rec.kind, rec.w, rec.h = v.kind, v.w, v.h
        rec.m[:] = [float(x) for x in v.mat.reshape(-1)]
        rec.p[:] = list(v.params)
    mosaic = _lib.ViewMosaic()
    mosaic.low[:] = list(geom.low)
    mosaic.res[:] = list(geom.resolution)
    mosaic.h, mosaic.w = geom.shape
    mosaic.closed = 1 if geom.closed else 0
    return table, mosaic


def render_device(mosaic_or_mips, geom, views, eng=None):
    """Renders ``views`` (one launch) of a mosaic with geometry ``geom``: returns (images, masks),
    lists of uint8 device tensors [h][w][3] and [h][w] (1 = the mosaic covers the direction;
    uncovered pixels are 0 in both).  ``mosaic_or_mips``: ``Mips``, or a mosaic whose chain is
    built first.  Queued on the engine's stream."""
    import torch
    views = list(views)
    shape = mosaic_or_mips.shape if isinstance(mosaic_or_mips, Mips) else None
    if shape is None:
        _check_mosaic(mosaic_or_mips)
        shape = tuple(mosaic_or_mips.shape[:2])
    table, record = view_records(views, geom, tuple(shape))
    eng = _lib._engine(eng)
    dev = torch.device(eng.device)
    mips = mosaic_or_mips if isinstance(mosaic_or_mips, Mips) else mip_device(mosaic_or_mips, eng)
    images = [torch.empty((v.h, v.w, 3), dtype=torch.uint8, device=dev) for v in views]
    masks = [torch.empty((v.h, v.w), dtype=torch.uint8, device=dev) for v in views]
    for rec, img, mask in zip(table, images, masks):
        rec.image, rec.mask = img.data_ptr(), mask.data_ptr()
    offs = (C.c_int64 * len(mips.offsets))(*mips.offsets)
    eng.call("pano_view_render", mips.buffer, offs, mips.n_levels, C.byref(record), table,
             len(views))
    return images, masks


# ------------------------------------------------------------- host wrappers
def mip(mosaic, eng=None):
    """``mip_device`` on a host array: the levels as NumPy arrays."""
    mips = mip_device(np.asarray(mosaic), eng)
    return [mips.level(l).cpu().numpy() for l in range(mips.n_levels)]


def render(mosaic, geom, views, eng=None):
    """``render_device`` on a host mosaic: (images, masks) as lists of NumPy arrays."""
    images, masks = render_device(np.asarray(mosaic), geom, views, eng)
    return [t.cpu().numpy() for t in images], [t.cpu().numpy() for t in masks]
