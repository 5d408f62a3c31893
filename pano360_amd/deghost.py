"""Deghosting of exposure brackets before they are fused, on the device (``pano_deghost_u8``,
csrc/deghost.hip).

A bracket takes a second or more to shoot, and in a sweep something nearly always moves between
the exposures - a person, a car, leaves.  Exposure fusion then blends K different scenes: the
object appears K times, half transparent.  ``deghost_device`` makes the K exposures show ONE scene,
the reference exposure's, each still at its own exposure.  Two exposures of a static scene differ
by a monotone map of brightness, so a pixel's rank within its own frame's histogram is nearly the
same in both; a pixel whose rank disagrees with the reference's shows other content and is replaced
by the reference's pixel, carried to the exposure's brightness through the histogram-matching map
of the two frames, per colour channel.  A clipped pixel sits in a huge bin: its rank is an interval
that agrees with anything in it, so clipping needs no thresholds of its own.  The raw mask is eroded
(specks of noise, the thin lines a sub-pixel misalignment leaves on edges) and dilated (the
object's soft rim).  No exposure times, no EXIF and no floating point are needed.  The arithmetic
is stated in include/pano360.h and, in NumPy, in tests/deghost_model.py; the device returns it bit
for bit.  There is no CPU fallback.

Not covered: a mover whose brightness rank equals the background's is not seen; the replacement
always comes from the reference, so where the reference is clipped the detail of the other
exposures is lost inside the ghost region; no choice of the best-exposed source per region.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import fuse as _fuse

MAX_EXPOSURES = _fuse.MAX_EXPOSURES
MAX_SIDE = _fuse.MAX_SIDE
WARN_SHARE = 0.25


class DeghostParams:
    """``slack`` (0 .. 15): grey levels of noise tolerated; ``tol`` (0 .. 255): rank units of 1/255
    tolerated; ``erode`` (0 .. 3) and ``dilate`` (0 .. 15): the radii of the mask's clean-up;
    ``reference``: the exposure the others are made to agree with, None for exposure ``k // 2`` in
    file order - the middle exposure of the usual -/0/+ bracket."""
    __slots__ = ("slack", "tol", "erode", "dilate", "reference")
    _LIMITS = (("slack", 15), ("tol", 255), ("erode", 3), ("dilate", 15))

    def __init__(self, slack=3, tol=8, erode=1, dilate=3, reference=None):
        self.slack, self.tol, self.erode, self.dilate = int(slack), int(tol), int(erode), int(dilate)
        for name, top in self._LIMITS:
            if not 0 <= getattr(self, name) <= top:
                raise ValueError(f"{name} {getattr(self, name)} (0 .. {top})")
        if reference is not None and int(reference) < 0:
            raise ValueError(f"reference {reference}: None or >= 0")
        self.reference = None if reference is None else int(reference)

    def reference_of(self, k):
        return k // 2 if self.reference is None else self.reference

    def __repr__(self):
        return (f"DeghostParams({self.slack}, {self.tol}, {self.erode}, {self.dilate}, "
                f"reference={self.reference})")


def _check_stack(i, stack, params):
    stack = _fuse._check_stack(i, stack)                # (the same stacks the fusion takes)
    if params.reference_of(len(stack)) >= len(stack):
        raise ValueError(f"stack {i}: reference {params.reference} of {len(stack)} exposures")
    return stack


def _run(stacks, params, eng, apply, want_stages):
    """The one native call.  Returns the device copies of the stacks, the per-stack dst lists
    (None where nothing was asked for), the host counts and the stage outputs."""
    import torch
    params = params or DeghostParams()
    stacks = [_check_stack(i, stack, params) for i, stack in enumerate(stacks)]
    if not stacks:
        return [], [], [], []
    eng = _lib._engine(eng)
    records = (_lib.DeghostStack * len(stacks))()
    device = torch.device(eng.device)
    counts = torch.empty(sum(len(s) for s in stacks), dtype=torch.int32, device=device)
    keep, dsts, debug = [], [], []
    need, at = 0, 0
    for rec, stack in zip(records, stacks):
        stack = [_lib.rgb_on_device(frame, eng) for frame in stack]
        keep.append(stack)
        h, w, k = int(stack[0].shape[0]), int(stack[0].shape[1]), len(stack)
        rec.w, rec.h, rec.k, rec.reference = w, h, k, params.reference_of(k)
        out = [None] * k
        for e, frame in enumerate(stack):
            rec.src[e], rec.src_pitch[e] = frame.data_ptr(), frame.stride(0)
            if apply and e != rec.reference:
                out[e] = torch.empty((h, w, 3), dtype=torch.uint8, device=device)
                rec.dst[e], rec.dst_pitch[e] = out[e].data_ptr(), out[e].stride(0)
        dsts.append(out)
        rec.counts = counts[at:at + k].data_ptr()
        at += k
        if want_stages:
            wpr = (w + 31) // 32
            stage = {"hists": torch.empty((k, 4, 256), dtype=torch.int32, device=device),
                     "ranks": torch.empty((k, 2, 256), dtype=torch.uint8, device=device),
                     "maps": torch.empty((k, 3, 256), dtype=torch.uint8, device=device),
                     "raw": torch.empty((k, h, wpr), dtype=torch.int32, device=device),
                     "mask": torch.empty((k, h, wpr), dtype=torch.int32, device=device)}
            for name, t in stage.items():
                setattr(rec, name, t.data_ptr())
            debug.append(stage)
        need += int(eng.lib.pano_deghost_work_bytes(h, w, k))
    work = torch.empty(need, dtype=torch.uint8, device=device)
    native = _lib.DeghostParams(params.slack, params.tol, params.erode, params.dilate)
    eng.call("pano_deghost_u8", records, len(stacks), C.byref(native), work, need)
    host = counts.cpu().numpy()                         # (the one wait: the caller needs the counts)
    out_counts, at = [], 0
    for stack in keep:
        out_counts.append(host[at:at + len(stack)].copy())
        at += len(stack)
    return keep, dsts, out_counts, [_stages_of(d) for d in debug]


def _stages_of(stage):
    """The stage outputs of a stack as NumPy arrays, the counters and the bitmaps unsigned."""
    out = {name: t.cpu().numpy() for name, t in stage.items()}
    for name in ("hists", "raw", "mask"):
        out[name] = out[name].view(np.uint32)
    return out


def masks_device(stacks, params=None, eng=None, want_stages=False):
    """The ghost masks of every stack of ``stacks`` - a list of lists of 2 .. 8 uint8 [h][w][3] BGR
    device tensors of one size per stack, any sizes and counts across stacks - found in ONE native
    call: per stack a host int32 array [k], the pixels of each exposure that differ from the
    reference's scene (0 for the reference).  Rows may be further apart than 3 w bytes.  With
    ``want_stages`` a second list of dicts per stack: ``hists`` uint32 [k][4][256] (g, B, G, R),
    ``ranks`` uint8 [k][2][256] (lo, hi), ``maps`` uint8 [k][3][256], ``raw`` and ``mask`` uint32
    [k][h][ceil(w / 32)], packed.  ``ValueError`` for mixed sizes in a stack, a count outside
    2 .. 8, a wrong dtype or shape, or a reference that is no exposure of a stack."""
    _, _, counts, stages = _run(stacks, params, eng, False, want_stages)
    return (counts, stages) if want_stages else counts


def deghost_device(stacks, params=None, eng=None):
    """Deghosts every stack in ONE native call and returns ``(stacks, counts)``: the stacks with
    every changed exposure replaced by a new tensor - the reference and exposures with a count of
    0 are the very tensors that came in -, and the counts as ``masks_device`` returns them."""
    keep, dsts, counts, _ = _run(stacks, params, eng, True, False)
    out = [[dst if dst is not None and c > 0 else frame for frame, dst, c in zip(stack, ds, cs)]
           for stack, ds, cs in zip(keep, dsts, counts)]
    return out, counts


def deghost(stacks, params=None):
    """``deghost_device`` on host arrays: a list of lists of uint8 [h][w][3] NumPy arrays in, the
    deghosted NumPy arrays and the counts out."""
    out, counts = deghost_device([[np.asarray(f) for f in s] for s in stacks], params)
    return [[t.cpu().numpy() for t in stack] for stack in out], counts
