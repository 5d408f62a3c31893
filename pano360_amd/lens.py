"""Lens correction at the ingest, on the device (``pano_lens_undistort_u8``, csrc/lens.hip).

Everything behind the ingest assumes an ideal pinhole camera whose principal point is the image
centre: the warp's inverse map, the bundle adjuster's one focal length per camera, RANSAC's
homographies.  A calibrated camera is brought to that model here, once per frame and before
anything else looks at it: ``undistort_device`` resamples each decoded frame into the centred
pinhole image of a new focal length through the calibration's forward model - OpenCV's
``calibrateCamera`` coefficients (k1 k2 p1 p2 k3, ``"brown"``) or ``fisheye.calibrate``'s
(k1 .. k4, ``"fisheye"``) -, so nothing is iterated.  The arithmetic is stated in
include/pano360.h and, in NumPy, in tests/lens_model.py.  There is no CPU fallback.

``fit_focal`` chooses the new focal length so that the corrected frame holds only real pixels:
the stitch has no per-frame mask and blends whatever the frame's rectangle holds.  It takes the
distortion's radial profile as monotone over the frame (a calibration whose polynomial folds back
inside the frame is not a usable one), and it keeps the frame's size, so a wide fisheye loses
field of view: what a rectilinear image of that size cannot show is cropped.  Keeping that field
needs a fisheye term in the warp itself, which is a different, later piece of work.
Vignetting and chromatic aberration are out of scope; ``bundle_adj.refine`` estimates k1 and k2
from the matches and hands them over as ``LensModel`` records (``Refinement.lens_models``).
"""
import json
import logging
import os

import numpy as np

from . import _lib

KINDS = {"brown": _lib.LENS_BROWN, "fisheye": _lib.LENS_FISHEYE}
INTERPS = {"cubic": _lib.LENS_CUBIC, "linear": _lib.LENS_LINEAR}
COEFFICIENTS = {"brown": 5, "fisheye": 4}
MAX_SIDE = _lib.LENS_MAX_SIDE
MODEL_KEYS = ("model", "fx", "fy", "cx", "cy", "k", "size")


class LensModel:
    """One camera's calibration: ``kind`` "brown" (``k`` = k1 k2 p1 p2 k3, missing ones zero) or
    "fisheye" (``k`` = k1 k2 k3 k4), the camera matrix ``fx, fy, cx, cy`` in pixels and the
    resolution ``size = (w, h)`` the calibration holds for."""
    __slots__ = ("kind", "fx", "fy", "cx", "cy", "k", "size")

    def __init__(self, kind, fx, fy, cx, cy, k=(), size=None):
        if kind not in KINDS:
            raise ValueError(f"model {kind!r}: 'brown' or 'fisheye'")
        k = tuple(float(v) for v in k)
        count = COEFFICIENTS[kind]
        if len(k) > count or (kind == "fisheye" and len(k) != count):
            raise ValueError(f"k: {len(k)} coefficients for a {kind} model "
                             f"({'up to 5: k1 k2 p1 p2 k3' if kind == 'brown' else '4: k1 .. k4'})")
        if size is None or len(size) != 2:
            raise ValueError("size: (w, h), the resolution the calibration holds for")
        w, h = (int(v) for v in size)
        if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE) or (w, h) != tuple(size):
            raise ValueError(f"size {tuple(size)}: whole sides of 1 .. {MAX_SIDE}")
        self.kind, self.size = kind, (w, h)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.k = k + (0.0,) * (5 - len(k))
        for key in ("fx", "fy", "cx", "cy"):
            if not np.isfinite(getattr(self, key)):
                raise ValueError(f"{key}: {getattr(self, key)} is not finite")
        if not np.all(np.isfinite(self.k)):
            raise ValueError(f"k: {k} is not finite")
        if not (self.fx > 0 and self.fy > 0):
            raise ValueError(f"fx, fy: {self.fx}, {self.fy} are not positive")

    def __repr__(self):
        return (f"LensModel({self.kind!r}, fx={self.fx}, fy={self.fy}, cx={self.cx}, cy={self.cy}, "
                f"k={self.k[:COEFFICIENTS[self.kind]]}, size={self.size})")

    def project(self, u, v, f_new):
        """Where the output pixels (``u``, ``v``) of the corrected frame of focal length ``f_new``
        lie in the calibrated frame: float64 (px, py), not clamped."""
        w, h = self.size
        x = (np.asarray(u, np.float64) - w / 2.0) / f_new
        y = (np.asarray(v, np.float64) - h / 2.0) / f_new
        if self.kind == "brown":
            k1, k2, p1, p2, k3 = self.k
            r2 = x * x + y * y
            rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
            xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        else:
            k1, k2, k3, k4 = self.k[:4]
            r = np.sqrt(x * x + y * y)
            th = np.arctan(r)
            t2 = th * th
            thd = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            s = np.divide(thd, r, out=np.ones_like(r), where=r > 0)
            xd, yd = x * s, y * s
        return self.fx * xd + self.cx, self.fy * yd + self.cy


# ------------------------------------------------------------------ files
def _model_of(record, where):
    if not isinstance(record, dict):
        raise ValueError(f"{where}: a JSON object with the keys {', '.join(MODEL_KEYS)}")
    for key in record:
        if key not in MODEL_KEYS:
            raise ValueError(f"{where}: unknown key {key!r}")
    for key in MODEL_KEYS:
        if key not in record:
            raise ValueError(f"{where}: missing key {key!r}")
    try:
        return LensModel(record["model"], record["fx"], record["fy"], record["cx"], record["cy"],
                         record["k"], record["size"])
    except (TypeError, ValueError) as err:
        raise ValueError(f"{where}: {err}") from None


class Calibration:
    """The calibrations of a directory of frames: one model per file name (``cameras``) and a
    ``default`` for every other file; ``interp`` and ``focal`` are what ``undistort_device`` gets
    when the ingest applies it."""

    def __init__(self, default=None, cameras=None, interp="cubic", focal=None):
        self.default, self.cameras = default, dict(cameras or {})
        self.interp, self.focal = interp, focal
        if default is None and not self.cameras:
            raise ValueError("a calibration without a model")

    def model_for(self, name):
        model = self.cameras.get(os.path.basename(name), self.default)
        if model is None:
            raise ValueError(f"cameras: no calibration for {os.path.basename(name)!r} and no 'default'")
        return model

    def correct_device(self, frames, names, eng=None):
        """The ingest's step: ``undistort_device`` of the decoded ``frames`` of the files
        ``names``; logs every frame's focal length."""
        models = [self.model_for(name) for name in names]
        frames, focals = undistort_device(frames, models, self.interp, self.focal, eng)
        for name, focal in zip(names, focals):
            logging.info(f"Lens correction of {os.path.basename(name)}: focal length {focal:.6f}")
        return frames


def load(path):
    """The ``Calibration`` of a JSON file: either one model for every frame,
    ``{"model": "brown" | "fisheye", "fx": .., "fy": .., "cx": .., "cy": .., "k": [..],
    "size": [w, h]}``, or ``{"default": {model}, "cameras": {"<file name>": {model}}}`` (either
    key may be left out).  A ``ValueError`` names the offending key."""
    with open(path) as fid:
        record = json.load(fid)
    if not isinstance(record, dict):
        raise ValueError(f"{path}: a JSON object")
    if "default" not in record and "cameras" not in record:
        return Calibration(_model_of(record, path))
    for key in record:
        if key not in ("default", "cameras"):
            raise ValueError(f"{path}: unknown key {key!r} beside 'default' / 'cameras'")
    cameras = record.get("cameras", {})
    if not isinstance(cameras, dict):
        raise ValueError(f"{path}: 'cameras': a JSON object of file names")
    default = _model_of(record["default"], f"{path}: 'default'") if "default" in record else None
    try:
        return Calibration(default, {name: _model_of(rec, f"{path}: 'cameras': {name!r}")
                                     for name, rec in cameras.items()})
    except ValueError as err:
        raise ValueError(f"{path}: {err}") if "without a model" in str(err) else err


# --------------------------------------------------------------- the focal
def _border(w, h):
    """(u, v) of the border pixels of a w x h frame."""
    u, v = np.arange(w), np.arange(h)
    return (np.concatenate([u, u, np.zeros(h, int), np.full(h, w - 1)]),
            np.concatenate([np.zeros(w, int), np.full(w, h - 1), v, v]))


def fit_focal(model, size=None):
    """The smallest focal length of the corrected ``size = (w, h)`` frame (default: the model's)
    at which every border pixel maps into [0, w - 1] x [0, h - 1] of the calibrated frame: the
    corrected frame then holds only real pixels.  60 bisection steps on [f / 16, 16 f],
    f = (fx + fy) / 2, in float64; the bracket's upper end is returned, so the condition holds at
    the returned value itself.

    The radial profile is taken as monotone: then a larger focal length pulls every position
    towards the principal point, the condition is monotone in the focal length, and the border
    decides for the interior.  A wide fisheye loses field of view this way (see the module's
    text).  ``ValueError`` when the principal point lies outside the frame or the bracket's ends
    do not straddle (nothing fits even at 16 f, or everything already at f / 16)."""
    w, h = model.size if size is None else (int(size[0]), int(size[1]))
    if not (0 <= model.cx <= w - 1 and 0 <= model.cy <= h - 1):
        raise ValueError(f"the principal point ({model.cx}, {model.cy}) lies outside the "
                         f"{w} x {h} frame")
    u, v = _border(w, h)
    shaped = LensModel(model.kind, model.fx, model.fy, model.cx, model.cy,
                       model.k[:COEFFICIENTS[model.kind]], (w, h))

    def fits(focal):
        px, py = shaped.project(u, v, focal)
        return bool(np.all((px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)))

    f = (model.fx + model.fy) / 2
    low, high = f / 16, 16 * f
    if fits(low) or not fits(high):
        raise ValueError(f"no focal length in [{low}, {high}] separates a corrected {w} x {h} frame "
                         "that fits the calibrated one from one that does not")
    for _ in range(60):
        mid = (low + high) / 2
        if fits(mid):
            high = mid
        else:
            low = mid
    return float(high)


# ------------------------------------------------------------ the correction
def _focals(models, focal):
    if focal is None:
        return [fit_focal(m) for m in models]
    if np.ndim(focal) == 0:
        return [float(focal)] * len(models)
    if len(focal) != len(models):
        raise ValueError(f"{len(focal)} focal lengths for {len(models)} frames")
    return [fit_focal(m) if f is None else float(f) for m, f in zip(models, focal)]


def undistort_device(frames, models, interp="cubic", focal=None, eng=None):
    """Corrects a list of uint8 [h][w][3] device tensors (rows may be further apart than 3 w
    bytes: a rectangle of a larger tensor needs no copy) by ``models``, one ``LensModel`` or one
    per frame, in ONE native call.  ``interp`` "cubic" (Catmull-Rom) or "linear"; ``focal`` None:
    ``fit_focal`` per frame; a number or a list of numbers overrides it, and positions outside the
    calibrated frame then replicate its edge.  Returns (new device tensors, focal lengths).
    ``ValueError`` when a frame's size is not its model's.  Queued on the engine's stream."""
    import torch
    frames = list(frames)
    if isinstance(models, LensModel):
        models = [models] * len(frames)
    models = list(models)
    if len(models) != len(frames):
        raise ValueError(f"{len(models)} models for {len(frames)} frames")
    if interp not in INTERPS:
        raise ValueError(f"interp {interp!r}: 'cubic' or 'linear'")
    for i, (frame, model) in enumerate(zip(frames, models)):
        shape = tuple(frame.shape)
        if not _lib.is_rgb_u8(frame):
            raise ValueError(f"frame {i}: {frame.dtype} {shape}, not uint8 [h][w][3]")
        if (shape[1], shape[0]) != model.size:
            raise ValueError(f"frame {i} is {shape[1]} x {shape[0]}, its calibration holds for "
                             f"{model.size[0]} x {model.size[1]}")
    focals = _focals(models, focal)
    if not frames:
        return [], []
    eng = _lib._engine(eng)
    records = (_lib.LensFrame * len(frames))()
    sources, outs = [], []
    for rec, frame, model, f_new in zip(records, frames, models, focals):
        frame = _lib.rgb_on_device(frame, eng)
        h, w = int(frame.shape[0]), int(frame.shape[1])
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=frame.device)
        rec.src, rec.dst = frame.data_ptr(), out.data_ptr()
        rec.src_pitch, rec.dst_pitch = frame.stride(0), out.stride(0)
        rec.fx, rec.fy, rec.cx, rec.cy, rec.f_new = model.fx, model.fy, model.cx, model.cy, f_new
        rec.k[:] = model.k
        rec.w, rec.h, rec.model, rec.interp = w, h, KINDS[model.kind], INTERPS[interp]
        sources.append(frame)
        outs.append(out)
    eng.call("pano_lens_undistort_u8", records, len(frames))
    return outs, focals


def undistort(frames, models, interp="cubic", focal=None, eng=None):
    """``undistort_device`` on host arrays: (corrected NumPy arrays, focal lengths)."""
    outs, focals = undistort_device([np.asarray(f) for f in frames], models, interp, focal, eng)
    return [t.cpu().numpy() for t in outs], focals


# ------------------------------------------------------------- command line
def add_arguments(parser):
    """``--lens``, ``--lens-interp`` and ``--lens-focal`` of stitcher.py and features.py."""
    parser.add_argument("--lens", type=str, metavar="FILE",
                        help="correct the lens distortion of every image as it is read, on the "
                             "device, by the calibration in this JSON file (one model, or "
                             "'default' and 'cameras' by file name; OpenCV's coefficients, for "
                             "the files' own resolution); the caches get a _lens suffix.")
    parser.add_argument("--lens-interp", choices=list(INTERPS), default=None,
                        help="--lens: the resampling filter (default cubic).")
    parser.add_argument("--lens-focal", type=float, metavar="FLOAT", default=None,
                        help="--lens: the corrected images' focal length in pixels, instead of the "
                             "smallest one that leaves no empty border (what falls outside then "
                             "repeats the edge).")


def check_arguments(parser, args):
    if args.lens is None and (args.lens_interp is not None or args.lens_focal is not None):
        parser.error("--lens-interp and --lens-focal need --lens")
    if args.lens_focal is not None and not (np.isfinite(args.lens_focal) and args.lens_focal > 0):
        parser.error("--lens-focal: a positive number")


def from_args(args):
    """The ``Calibration`` the command line asks for (None without ``--lens``)."""
    if args.lens is None:
        return None
    calibration = load(args.lens)
    calibration.interp = args.lens_interp or "cubic"
    calibration.focal = args.lens_focal
    return calibration
