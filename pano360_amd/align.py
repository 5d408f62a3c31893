"""Alignment of hand-held exposure brackets before they are fused, on the device
(``pano_align_mtb``, csrc/align.hip).

The exposures of a bracket shot hand-held or on a pole differ by a few pixels to a few dozen, and
exposure fusion of misaligned frames doubles every edge.  ``align_device`` finds an integer
translation of every exposure onto the stack's reference exposure by Ward's median threshold
bitmaps (G. Ward, "Fast, robust image registration for compositing high dynamic range photographs
from hand-held exposures", 2003; OpenCV's ``AlignMTB``): each exposure becomes a bitmap "brighter
than its own median", which hardly depends on the exposure, and the translation is found coarse to
fine over a pyramid of such bitmaps by counting differing bits, pixels close to the median left
out.  No exposure times, no features and no floating point are needed.  The frames are then copied
shifted, the border replicated.  The arithmetic is stated in include/pano360.h and, in NumPy, in
tests/align_model.py; the device returns it bit for bit.  There is no CPU fallback.

``levels_for(h, w, max_bits)`` levels above the frame are searched, so that the coarsest keeps a
short side of at least 16, and a shift of up to ``2 ** (L + 1) - 1`` pixels is found: 127 from a
short side of 1024 on with the default ``max_bits`` of 6.

Not covered: rotation and parallax between the exposures, sub-pixel shifts, and what moved in the
scene.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import fuse as _fuse

MAX_EXPOSURES = _fuse.MAX_EXPOSURES
MAX_SIDE = _fuse.MAX_SIDE
MAX_BITS = 7


def levels_for(h, w, max_bits=6):
    """The levels above an h x w frame: ``min(max_bits, max(0, bit_length(min(h, w)) - 5))``."""
    return min(int(max_bits), max(0, int(min(h, w)).bit_length() - 5))


def reach_for(h, w, max_bits=6):
    """The largest shift the search can return: ``2 ** (L + 1) - 1``."""
    return 2 ** (levels_for(h, w, max_bits) + 1) - 1


class AlignParams:
    """``max_bits`` (0 .. 7): at most this many levels above the frame; ``exclude`` (0 .. 127):
    pixels this close to their frame's median are left out; ``reference``: the exposure the others
    are moved onto, None for exposure ``k // 2`` in file order - the middle exposure of the usual
    -/0/+ bracket."""
    __slots__ = ("max_bits", "exclude", "reference")

    def __init__(self, max_bits=6, exclude=4, reference=None):
        self.max_bits, self.exclude = int(max_bits), int(exclude)
        if not 0 <= self.max_bits <= MAX_BITS:
            raise ValueError(f"max_bits {max_bits} (0 .. {MAX_BITS})")
        if not 0 <= self.exclude <= 127:
            raise ValueError(f"exclude {exclude} (0 .. 127)")
        if reference is not None and int(reference) < 0:
            raise ValueError(f"reference {reference}: None or >= 0")
        self.reference = None if reference is None else int(reference)

    def reference_of(self, k):
        return k // 2 if self.reference is None else self.reference

    def __repr__(self):
        return f"AlignParams({self.max_bits}, {self.exclude}, reference={self.reference})"


def _check_stack(i, stack, params):
    stack = _fuse._check_stack(i, stack)                # (the same stacks the fusion takes)
    if params.reference_of(len(stack)) >= len(stack):
        raise ValueError(f"stack {i}: reference {params.reference} of {len(stack)} exposures")
    return stack


def _level_shapes(h, w, levels):
    """(h_l, w_l, words per bitmap row) of the levels 0 .. L."""
    return [(h >> l, w >> l, ((w >> l) + 31) // 32) for l in range(levels + 1)]


def _run(stacks, params, eng, apply, want_stages):
    """The one native call.  Returns the device copies of the stacks, the per-stack dst lists
    (None where nothing was asked for), the host shifts and the stage outputs."""
    import torch
    params = params or AlignParams()
    stacks = [_check_stack(i, stack, params) for i, stack in enumerate(stacks)]
    if not stacks:
        return [], [], [], []
    eng = _lib._engine(eng)
    records = (_lib.AlignStack * len(stacks))()
    device = torch.device(eng.device)
    total_k = sum(len(s) for s in stacks)
    shifts = torch.empty((total_k, 2), dtype=torch.int32, device=device)
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
        rec.shifts = shifts[at:at + k].data_ptr()
        at += k
        if want_stages:
            shapes = _level_shapes(h, w, levels_for(h, w, params.max_bits))
            grey = torch.empty(k * sum(a * b for a, b, _ in shapes), dtype=torch.uint8, device=device)
            medians = torch.empty((k, len(shapes)), dtype=torch.int32, device=device)
            bitmaps = torch.empty(k * sum(2 * a * c for a, _, c in shapes), dtype=torch.int32, device=device)
            errs = torch.empty((k, len(shapes), 9), dtype=torch.int32, device=device)
            rec.grey, rec.medians, rec.bitmaps, rec.errs = (t.data_ptr() for t in (grey, medians, bitmaps, errs))
            debug.append((shapes, grey, medians, bitmaps, errs))
        need += int(eng.lib.pano_align_work_bytes(h, w, k))
    work = torch.empty(need, dtype=torch.uint8, device=device)
    native = _lib.AlignParams(params.max_bits, params.exclude)
    eng.call("pano_align_mtb", records, len(stacks), C.byref(native), work, need)
    host = shifts.cpu().numpy()                         # (the one wait: the caller needs the shifts)
    out_shifts, at = [], 0
    for stack in keep:
        out_shifts.append(host[at:at + len(stack)].copy())
        at += len(stack)
    return keep, dsts, out_shifts, [_stages_of(len(s), *d) for s, d in zip(keep, debug)]


def _stages_of(k, shapes, grey, medians, bitmaps, errs):
    """The dense stage outputs of a stack cut into per-frame, per-level NumPy arrays."""
    grey, bitmaps = grey.cpu().numpy(), bitmaps.cpu().numpy().view(np.uint32)
    out = {"grey": [], "tb": [], "eb": [], "medians": medians.cpu().numpy(),
           "err": errs.cpu().numpy().view(np.uint32)}
    g_at = b_at = 0
    for _ in range(k):
        g, t, e = [], [], []
        for h, w, wpr in shapes:
            g.append(grey[g_at:g_at + h * w].reshape(h, w))
            t.append(bitmaps[b_at:b_at + h * wpr].reshape(h, wpr))
            e.append(bitmaps[b_at + h * wpr:b_at + 2 * h * wpr].reshape(h, wpr))
            g_at, b_at = g_at + h * w, b_at + 2 * h * wpr
        out["grey"].append(g), out["tb"].append(t), out["eb"].append(e)
    return out


def shifts_device(stacks, params=None, eng=None, want_stages=False):
    """The integer shifts of every stack of ``stacks`` - a list of lists of 2 .. 8 uint8 [h][w][3]
    BGR device tensors of one size per stack, any sizes and counts across stacks - found in ONE
    native call: per stack a host int32 array [k][2] of (dx, dy), (0, 0) for the reference;
    ``aligned[y][x] = src[y - dy][x - dx]``.  Rows may be further apart than 3 w bytes.  With
    ``want_stages`` a second list of dicts per stack: ``grey``, ``tb`` and ``eb`` as [k][L + 1]
    NumPy arrays (the bitmaps packed, uint32 [h_l][ceil(w_l / 32)]), ``medians`` int32 [k][L + 1]
    and ``err`` uint32 [k][L + 1][9].  ``ValueError`` for mixed sizes in a stack, a count outside
    2 .. 8, a wrong dtype or shape, or a reference that is no exposure of a stack."""
    _, _, shifts, stages = _run(stacks, params, eng, False, want_stages)
    return (shifts, stages) if want_stages else shifts


def align_device(stacks, params=None, eng=None):
    """Aligns every stack in ONE native call and returns ``(aligned, shifts)``: the stacks with
    every moved exposure replaced by its shifted copy (the border replicated) - the reference and
    exposures whose shift is (0, 0) are the very tensors that came in -, and the shifts as
    ``shifts_device`` returns them."""
    keep, dsts, shifts, _ = _run(stacks, params, eng, True, False)
    aligned = [[dst if dst is not None and s.any() else frame for frame, dst, s in zip(stack, out, sh)]
               for stack, out, sh in zip(keep, dsts, shifts)]
    return aligned, shifts


def align(stacks, params=None):
    """``align_device`` on host arrays: a list of lists of uint8 [h][w][3] NumPy arrays in, the
    aligned NumPy arrays and the shifts out."""
    aligned, shifts = align_device([[np.asarray(f) for f in s] for s in stacks], params)
    return [[t.cpu().numpy() for t in stack] for stack in aligned], shifts
