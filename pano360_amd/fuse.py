"""Exposure fusion of bracketed frames at the ingest, on the device (``pano_fuse_u8``,
csrc/fuse.hip).

A full sphere rarely fits one exposure - an interior with windows, a sun in the frame - and is
shot as exposure brackets: K exposures per tripod position.  ``fuse_device`` merges the K frames
of a position into one ordinary 8-bit frame before detection sees it, by the exposure fusion of
Mertens, Kautz and Van Reeth (2007; OpenCV's ``MergeMertens``): every pixel of every exposure gets
a weight from its local contrast, its saturation and its closeness to mid-grey, the weights are
normalised over the exposures, and the frames' Laplacian pyramids are summed under the weights'
Gaussian pyramids and collapsed.  No exposure times, no response curve and no EXIF are needed, and
nothing downstream changes: the result is a uint8 BGR frame.

Two choices differ from OpenCV's defaults.  The exponents default to the paper's ``(1, 1, 1)``
(contrast, saturation, well-exposedness); OpenCV's ``createMergeMertens`` defaults to
``(1, 1, 0)``, which ``FuseParams(exposure=0)`` gives.  And the pyramids have
``levels_for(h, w) = max(0, bit_length(min(h, w)) - 2)`` levels below the frame, one fewer than
OpenCV's ``int(log2(min side))``: the coarsest level stays at least 2 x 2, where ``pyrUp`` is
defined.  The arithmetic is stated in include/pano360.h and, in NumPy, in tests/fuse_model.py.
There is no CPU fallback.

The brackets are taken as aligned (a tripod) unless ``Bracket(k, align=AlignParams())`` /
``--bracket-align`` asks for the integer alignment of ``pano360_amd.align`` first, and what moved
in the scene between the exposures ghosts unless ``Bracket(k, deghost=DeghostParams())`` /
``--bracket-deghost`` asks for ``pano360_amd.deghost`` before the fusion.  Not covered: rotation
and parallax between the exposures, a radiance (HDR) output and tone mapping.
"""
import argparse
import ctypes as C
import logging
import os

import numpy as np

from . import _lib

MAX_EXPOSURES = _lib.FUSE_MAX_EXPOSURES
MAX_SIDE = _lib.FUSE_MAX_SIDE


def levels_for(h, w):
    """The pyramid levels below an h x w frame: ``max(0, bit_length(min(h, w)) - 2)``."""
    return max(0, int(min(h, w)).bit_length() - 2)


class FuseParams:
    """The exponents of the three quality measures (finite, >= 0; 1 takes the measure as it is, 0
    leaves it out) and ``n_levels``: None for ``levels_for`` of each stack, or 0 .. that."""
    __slots__ = ("contrast", "saturation", "exposure", "n_levels")

    def __init__(self, contrast=1.0, saturation=1.0, exposure=1.0, n_levels=None):
        self.contrast, self.saturation, self.exposure = float(contrast), float(saturation), float(exposure)
        for name in ("contrast", "saturation", "exposure"):
            value = getattr(self, name)
            if not (np.isfinite(value) and value >= 0):
                raise ValueError(f"{name} {value}: a finite exponent >= 0")
        if n_levels is not None and int(n_levels) < 0:
            raise ValueError(f"n_levels {n_levels}: None or >= 0")
        self.n_levels = None if n_levels is None else int(n_levels)

    def __repr__(self):
        return (f"FuseParams({self.contrast}, {self.saturation}, {self.exposure}, "
                f"n_levels={self.n_levels})")


def _check_stack(i, stack):
    stack = list(stack)
    if not 2 <= len(stack) <= MAX_EXPOSURES:
        raise ValueError(f"stack {i}: {len(stack)} exposures (2 .. {MAX_EXPOSURES})")
    for e, frame in enumerate(stack):
        shape = tuple(frame.shape)
        if not _lib.is_rgb_u8(frame):
            raise ValueError(f"stack {i}, exposure {e}: {frame.dtype} {shape}, not uint8 [h][w][3]")
        if shape != tuple(stack[0].shape):
            raise ValueError(f"stack {i}: exposure {e} is {shape[1]} x {shape[0]}, exposure 0 "
                             f"{stack[0].shape[1]} x {stack[0].shape[0]}")
    h, w = stack[0].shape[:2]
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"stack {i}: {w} x {h} (sides 1 .. {MAX_SIDE})")
    return stack


def fuse_device(stacks, params=None, eng=None, want_stages=False):
    """Fuses every stack of ``stacks`` - a list of lists of 2 .. 8 uint8 [h][w][3] BGR device
    tensors of one size per stack, any sizes and counts across stacks - in ONE native call, through
    one workspace sized for the largest.  Rows may be further apart than 3 w bytes (a rectangle of
    a larger tensor is passed by its pitch, not copied).  Returns the fused uint8 [h][w][3] device
    tensors; with ``want_stages`` a second list of ``(raw, fused_f32)`` per stack: the raw weights
    float32 [k][h][w] and the collapsed pyramid float32 [h][w][3] before it is quantised, written
    by the kernels that feed the next stage.  ``ValueError`` for mixed sizes in a stack, a count
    outside 2 .. 8, a wrong dtype or shape, or ``n_levels`` above a stack's ``levels_for``.
    Queued on the engine's stream."""
    import torch
    params = params or FuseParams()
    stacks = [_check_stack(i, stack) for i, stack in enumerate(stacks)]
    for i, stack in enumerate(stacks):
        h, w = stack[0].shape[:2]
        if params.n_levels is not None and params.n_levels > levels_for(h, w):
            raise ValueError(f"stack {i}: n_levels {params.n_levels}, {w} x {h} has at most "
                             f"{levels_for(h, w)}")
    if not stacks:
        return ([], []) if want_stages else []
    eng = _lib._engine(eng)
    records = (_lib.FuseStack * len(stacks))()
    keep, outs, stages = [], [], []
    need = 0
    for rec, stack in zip(records, stacks):
        stack = [_lib.rgb_on_device(frame, eng) for frame in stack]
        keep.append(stack)
        h, w, k = int(stack[0].shape[0]), int(stack[0].shape[1]), len(stack)
        device = stack[0].device
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=device)
        for e, frame in enumerate(stack):
            rec.src[e], rec.src_pitch[e] = frame.data_ptr(), frame.stride(0)
        rec.dst, rec.dst_pitch = out.data_ptr(), out.stride(0)
        rec.w, rec.h, rec.k = w, h, k
        if want_stages:
            raw = torch.empty((k, h, w), dtype=torch.float32, device=device)
            fused = torch.empty((h, w, 3), dtype=torch.float32, device=device)
            rec.raw, rec.fused = raw.data_ptr(), fused.data_ptr()
            stages.append((raw, fused))
        outs.append(out)
        need = max(need, int(eng.lib.pano_fuse_work_bytes(h, w, k)))
    work = torch.empty(need, dtype=torch.uint8, device=outs[0].device)
    native = _lib.FuseParams(params.contrast, params.saturation, params.exposure,
                             -1 if params.n_levels is None else params.n_levels)
    eng.call("pano_fuse_u8", records, len(stacks), C.byref(native), work, need)
    # (the kernels are queued on the stream the tensors belong to: the frames and `work` may go)
    return (outs, stages) if want_stages else outs


def fuse(stacks, params=None):
    """``fuse_device`` on host arrays: a list of lists of uint8 [h][w][3] NumPy arrays in, the
    fused NumPy arrays out."""
    return [t.cpu().numpy() for t in fuse_device([[np.asarray(f) for f in s] for s in stacks], params)]


def group_files(files, k):
    """The file names sorted and cut into consecutive groups of ``k``: the brackets of one
    position after another, as cameras number them.  ``ValueError`` when the count is no multiple
    of ``k``."""
    files, k = sorted(files), int(k)
    if not 2 <= k <= MAX_EXPOSURES:
        raise ValueError(f"brackets of {k} (2 .. {MAX_EXPOSURES})")
    if len(files) % k:
        raise ValueError(f"{len(files)} images cannot be grouped into brackets of {k}")
    return [files[i:i + k] for i in range(0, len(files), k)]


class Bracket:
    """What ``--bracket`` asked for: ``k`` exposures per position, the ``FuseParams``, ``align``:
    None for brackets that are aligned as they are, or the ``align.AlignParams`` of
    ``--bracket-align``, and ``deghost``: None for a scene in which nothing moves, or the
    ``deghost.DeghostParams`` of ``--bracket-deghost``."""
    __slots__ = ("k", "params", "align", "deghost")

    def __init__(self, k, params=None, align=None, deghost=None):
        self.k = int(k)
        if not 2 <= self.k <= MAX_EXPOSURES:
            raise ValueError(f"brackets of {self.k} (2 .. {MAX_EXPOSURES})")
        self.params = params or FuseParams()
        self.align = align
        self.deghost = deghost

    def fuse_groups(self, frames, groups, eng=None):
        """``frames``: the decoded device tensors in the order of the groups' files.  Every group
        fused by ONE ``fuse_device`` call - with ``align``, after ONE ``align.align_device`` call
        has moved the exposures of every group onto its reference; each bracket's shifts are
        logged under its first file name, with a warning for a shift at the search's limit; with
        ``deghost``, ONE ``deghost.deghost_device`` call then makes the exposures of every group
        show the scene of its reference (the one ``align`` used), and the share of pixels replaced
        in each exposure is logged, with a warning above a quarter of the frame.  A
        group whose frames differ in size is a ``ValueError`` that names its files."""
        stacks, at = [], 0
        for group in groups:
            stack = frames[at:at + len(group)]
            at += len(group)
            if len({tuple(f.shape) for f in stack}) != 1:
                sizes = ", ".join(f"{os.path.basename(n)} {f.shape[1]} x {f.shape[0]}"
                                  for n, f in zip(group, stack))
                raise ValueError(f"the exposures of a bracket differ in size: {sizes}")
            stacks.append(stack)
        if self.align is not None and stacks:
            from . import align as _align
            stacks, shifts = _align.align_device(stacks, self.align, eng)
            for group, stack, found in zip(groups, stacks, shifts):
                h, w = stack[0].shape[:2]
                reach = _align.reach_for(h, w, self.align.max_bits)
                name = os.path.basename(group[0])
                logging.info(f"Bracket alignment of {name}: (dx, dy) = {[tuple(int(v) for v in s) for s in found]}")
                if np.abs(found).max() >= reach:
                    logging.warning(f"Bracket alignment of {name}: a shift at the limit of {reach} pixels - "
                                    f"the exposures moved further than the search reaches")
        if self.deghost is not None and stacks:
            from . import deghost as _deghost
            how = self.deghost
            if self.align is not None:                  # (the exposure the others were moved onto)
                how = _deghost.DeghostParams(how.slack, how.tol, how.erode, how.dilate,
                                             self.align.reference_of(self.k))
            stacks, counts = _deghost.deghost_device(stacks, how, eng)
            for group, stack, found in zip(groups, stacks, counts):
                shares = [int(c) / (stack[0].shape[0] * stack[0].shape[1]) for c in found]
                name = os.path.basename(group[0])
                logging.info(f"Bracket deghosting of {name}: replaced {[round(v, 4) for v in shares]} of the pixels")
                if max(shares) > _deghost.WARN_SHARE:
                    logging.warning(f"Bracket deghosting of {name}: {max(shares):.2f} of an exposure differs from "
                                    f"the reference - misaligned exposures (--bracket-align) or a changed scene; "
                                    f"the result is mostly the reference exposure")
        return fuse_device(stacks, self.params, eng)


# ------------------------------------------------------------- command line
def _weights(text):
    try:
        values = [float(v) for v in text.split(",")]
    except ValueError:
        values = []
    if len(values) != 3 or not all(np.isfinite(v) and v >= 0 for v in values):
        raise argparse.ArgumentTypeError(f"{text!r}: three finite exponents >= 0, as C,S,E")
    return tuple(values)


def _bits(text):
    try:
        bits = int(text)
    except ValueError:
        bits = -1
    if not 0 <= bits <= 7:
        raise argparse.ArgumentTypeError(f"{text!r}: 0 .. 7 pyramid levels")
    return bits


def _tol(text):
    try:
        tol = int(text)
    except ValueError:
        tol = -1
    if not 0 <= tol <= 255:
        raise argparse.ArgumentTypeError(f"{text!r}: 0 .. 255 rank units of 1/255")
    return tol


def _count(text):
    try:
        k = int(text)
    except ValueError:
        k = 0
    if not 2 <= k <= MAX_EXPOSURES:
        raise argparse.ArgumentTypeError(f"{text!r}: 2 .. {MAX_EXPOSURES} exposures per position")
    return k


def add_arguments(parser):
    """``--bracket``, ``--bracket-weights``, ``--bracket-align``, ``--bracket-align-bits``,
    ``--bracket-deghost`` and ``--bracket-deghost-tol`` of stitcher.py and features.py.  Without
    the flags the parsed namespace is what it was (no attribute: ``bracket_of``, ``align_of`` and
    ``deghost_of`` read them)."""
    parser.add_argument("--bracket", type=_count, metavar="K", default=argparse.SUPPRESS,
                        help="the directory holds exposure brackets, K (2 .. 8) consecutive files "
                             "(in sorted order) per position: each bracket is fused into one frame "
                             "on the device as it is read (exposure fusion, Mertens et al.); the "
                             "caches get a _b<K> suffix.")
    parser.add_argument("--bracket-weights", type=_weights, metavar="C,S,E", default=argparse.SUPPRESS,
                        help="--bracket: the exponents of contrast, saturation and well-exposedness "
                             "(default 1,1,1, the paper's; OpenCV's default is 1,1,0).")
    parser.add_argument("--bracket-align", action="store_true", default=argparse.SUPPRESS,
                        help="--bracket: the brackets were shot hand-held: the exposures of each are "
                             "moved onto its middle one by an integer shift before they are fused "
                             "(median threshold bitmaps, Ward 2003); the caches get _b<K>a.")
    parser.add_argument("--bracket-align-bits", type=_bits, metavar="N", default=argparse.SUPPRESS,
                        help="--bracket-align: at most N (0 .. 7, default 6) pyramid levels: shifts "
                             "up to 2^(N+1) - 1 pixels are found.")
    parser.add_argument("--bracket-deghost", action="store_true", default=argparse.SUPPRESS,
                        help="--bracket: something moved in the scene between the exposures: where an "
                             "exposure's brightness ranks disagree with the middle exposure's, it takes "
                             "that exposure's pixels, carried to its own brightness, before the fusion "
                             "(after --bracket-align, if given); the caches get _b<K>g or _b<K>ag.")
    parser.add_argument("--bracket-deghost-tol", type=_tol, metavar="N", default=argparse.SUPPRESS,
                        help="--bracket-deghost: ranks may differ by N / 255 (0 .. 255, default 8) of "
                             "the frame's pixels before a pixel counts as moved.")


def bracket_of(args):
    """K of ``--bracket``, or None."""
    return getattr(args, "bracket", None)


def align_of(args):
    """True with ``--bracket-align``."""
    return bool(getattr(args, "bracket_align", False))


def deghost_of(args):
    """True with ``--bracket-deghost``."""
    return bool(getattr(args, "bracket_deghost", False))


def cache_suffix(args):
    """What the flags add to a cache name: nothing, or ``_b<K>`` and then ``a`` when aligned and
    ``g`` when deghosted: ``_b<K>``, ``_b<K>a``, ``_b<K>g``, ``_b<K>ag``."""
    if bracket_of(args) is None:
        return ""
    return f"_b{bracket_of(args)}" + ("a" if align_of(args) else "") + ("g" if deghost_of(args) else "")


def check_arguments(parser, args):
    if bracket_of(args) is None and getattr(args, "bracket_weights", None) is not None:
        parser.error("--bracket-weights needs --bracket")
    if bracket_of(args) is None and align_of(args):
        parser.error("--bracket-align needs --bracket")
    if not align_of(args) and getattr(args, "bracket_align_bits", None) is not None:
        parser.error("--bracket-align-bits needs --bracket-align")
    if bracket_of(args) is None and deghost_of(args):
        parser.error("--bracket-deghost needs --bracket")
    if not deghost_of(args) and getattr(args, "bracket_deghost_tol", None) is not None:
        parser.error("--bracket-deghost-tol needs --bracket-deghost")


def from_args(args):
    """The ``Bracket`` the command line asks for (None without ``--bracket``)."""
    if bracket_of(args) is None:
        return None
    weights = getattr(args, "bracket_weights", None) or (1.0, 1.0, 1.0)
    how = None
    if align_of(args):
        from . import align as _align
        how = _align.AlignParams(max_bits=getattr(args, "bracket_align_bits", 6))
    ghosts = None
    if deghost_of(args):
        from . import deghost as _deghost
        ghosts = _deghost.DeghostParams(tol=getattr(args, "bracket_deghost_tol", 8))
    return Bracket(bracket_of(args), FuseParams(*weights), how, ghosts)
