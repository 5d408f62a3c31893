"""Local alignment of the warped patches before the blend (``--local-align``; DESIGN.md section
5u, the contract in include/pano360.h).  Two overlapping frames that disagree by a small, smooth,
locally varying displacement - the parallax of a hand-held sweep - are each moved part of the way
towards the other, in proportion to the other's blend weight: a dense block-matching field per
pair of overlapping patches in mosaic space (coarse to fine, integers), smoothed by a median, and
one resampling of every patch that has a partner.  The masks do not change, so the valid area
and the crop rectangle are those of the stitch without it.  No reference counterpart."""
import copy
import ctypes as C
import logging

import numpy as np

from . import _lib


class FlowParams:
    """``levels``: 0 .. 4 pyramid levels above the pixels, a reach of ``2 ** (levels + 1) - 1``
    pixels; ``gain``: what a block must gain by leaving its inherited vector, in 1/16 grey levels
    per sample; ``min_overlap``: the side of the smallest intersection of two rects that is
    aligned."""

    def __init__(self, levels=3, gain=16, min_overlap=64):
        if not (isinstance(levels, (int, np.integer)) and 0 <= levels <= _lib.FLOW_MAX_LEVELS):
            raise ValueError(f"FlowParams: levels {levels!r} (0 .. {_lib.FLOW_MAX_LEVELS})")
        if not (isinstance(gain, (int, np.integer)) and 1 <= gain <= _lib.FLOW_MAX_GAIN):
            raise ValueError(f"FlowParams: gain {gain!r} (1 .. {_lib.FLOW_MAX_GAIN})")
        if not (isinstance(min_overlap, (int, np.integer)) and min_overlap >= 16):
            raise ValueError(f"FlowParams: min_overlap {min_overlap!r} (>= 16)")
        self.levels, self.gain, self.min_overlap = int(levels), int(gain), int(min_overlap)

    @property
    def reach(self):
        return 2 ** (self.levels + 1) - 1

    def native(self):
        return _lib.FlowParams(self.levels, self.gain, self.min_overlap, 0)

    def __repr__(self):
        return f"FlowParams({self.levels}, {self.gain}, {self.min_overlap})"


def pairs_for(rects, params=None):
    """[(i, j, L_ij, y0, y1, x0, x1)] of ``rects`` (y0, x0, h, w): every i < j whose rects meet in
    at least ``min_overlap`` x ``min_overlap`` pixels, the levels its search starts at and the
    intersection."""
    params = params or FlowParams()
    out = []
    for i, a in enumerate(rects):
        for j in range(i + 1, len(rects)):
            b = rects[j]
            y0, y1 = max(a[0], b[0]), min(a[0] + a[2], b[0] + b[2])
            x0, x1 = max(a[1], b[1]), min(a[1] + a[3], b[1] + b[3])
            if y1 - y0 < params.min_overlap or x1 - x0 < params.min_overlap:
                continue
            levels = min(params.levels, max(0, int(min(y1 - y0, x1 - x0)).bit_length() - 6))
            out.append((i, j, levels, int(y0), int(y1), int(x0), int(x1)))
    return out


def block_range(pair, level):
    """(by0, bx0, nby, nbx): the 16 x 16-sample blocks of a level that meet a pair's intersection."""
    _, _, _, y0, y1, x0, x1 = pair
    s = level + 4
    return y0 >> s, x0 >> s, ((y1 - 1) >> s) - (y0 >> s) + 1, ((x1 - 1) >> s) - (x0 >> s) + 1


def _a256(v):
    return (v + 255) // 256 * 256


class Layout:
    """The workspace of a call (include/pano360.h states it): where every camera's levels, every
    pair's block vectors and smoothed vectors and the statistics lie."""

    def __init__(self, rects, params):
        self.pairs = pairs_for(rects, params)
        self.top = max([p[2] for p in self.pairs], default=0)
        self.paired = [any(c in p[:2] for p in self.pairs) for c in range(len(rects))]
        at = 0
        self.gv = {}                # (camera, level) -> (byte offset, rows, columns, y0, x0 in samples)
        for c, (y0, x0, h, w) in enumerate(rects):
            if not self.paired[c]:
                continue
            ay0, ax0 = y0 & ~15, x0 & ~15
            bh, bw = ((y0 + h + 15) & ~15) - ay0, ((x0 + w + 15) & ~15) - ax0
            for l in range(self.top + 1):
                self.gv[c, l] = (at, bh >> l, bw >> l, ay0 >> l, ax0 >> l)
                at += 2 * (bh >> l) * (bw >> l)
        self.pyramid_bytes = at
        self.vectors_at = at = _a256(at)
        self.vec = {}               # (pair, level) -> (byte offset, nby, nbx)
        for q, pair in enumerate(self.pairs):
            for l in range(pair[2] + 1):
                _, _, nby, nbx = block_range(pair, l)
                self.vec[q, l] = (at, nby, nbx)
                at += 8 * nby * nbx
        self.vectors_bytes = at - self.vectors_at
        self.fields_at = at = _a256(at)
        self.smooth = {}            # pair -> (byte offset, nby, nbx)
        for q, pair in enumerate(self.pairs):
            _, _, nby, nbx = block_range(pair, 0)
            self.smooth[q] = (at, nby, nbx)
            at += 4 * nby * nbx
        self.fields_bytes = at - self.fields_at
        self.stats_at = _a256(at)
        self.total = self.stats_at + 256

    # views of a host copy of the workspace (uint8 [total])
    def level_of(self, work, c, l):
        at, rows, cols, _, _ = self.gv[c, l]
        return work[at:at + 2 * rows * cols].view(np.uint16).reshape(rows, cols)

    def vectors_of(self, work, q, l):
        at, nby, nbx = self.vec[q, l]
        return work[at:at + 8 * nby * nbx].view(np.int16).reshape(nby, nbx, 4)

    def field_of(self, work, q):
        at, nby, nbx = self.smooth[q]
        return work[at:at + 4 * nby * nbx].view(np.int16).reshape(nby, nbx, 2)

    def stats_of(self, work):
        return work[self.stats_at:self.stats_at + 16].view(np.int32)


def rects_of(patches):
    """(y0, x0, h, w) of stage-level device patches."""
    return [(int(p.rect[0]), int(p.rect[2]), int(p.h), int(p.w)) for p in patches]


def _table(patches, eng):
    from . import engine
    return engine.patch_table(patches, eng)


def _run(patches, shape, params, eng, apply, want_stages):
    """The one native call: (layout, output planes per patch or None, host workspace or None,
    host statistics)."""
    import torch
    params = params or FlowParams()
    eng = _lib._engine(eng)
    H, W = (int(v) for v in shape)
    table = _table(patches, eng)
    lay = Layout(rects_of(patches), params)
    native = params.native()
    need = int(eng.lib.pano_flow_work_bytes(table.host.ctypes.data_as(C.POINTER(_lib.Patch)), table.n,
                                            H, W, C.byref(native)))
    if need != lay.total:
        raise _lib.PanoError(f"flow: the library lays out {need} bytes, the package {lay.total}")
    device = torch.device(eng.device)
    work = torch.empty(need, dtype=torch.uint8, device=device)
    outs = [None] * len(patches)
    if apply:
        for c, p in enumerate(patches):
            if lay.paired[c]:
                outs[c] = torch.empty_like(p.planes)
                if p.pitch != p.w:
                    outs[c][:, :, p.w:] = 0
    ptrs = np.array([0 if t is None else t.data_ptr() for t in outs], np.uint64)
    stats = torch.zeros(4, dtype=torch.int32, device=device)
    if apply:
        eng.call("pano_flow_align", table.host, table.n, H, W, C.byref(native), work, need, ptrs,
                 None, None, None, stats)
    else:
        for stage in ("pano_flow_pyramid", "pano_flow_search", "pano_flow_smooth"):
            eng.call(stage, table.host, table.n, H, W, C.byref(native), work, need)
    host = None
    if want_stages or not apply:
        host = work.cpu().numpy()
    elif lay.pairs:                                     # the vectors alone, for the statistics
        host = np.zeros(need, np.uint8)
        host[lay.vectors_at:lay.stats_at] = work[lay.vectors_at:lay.stats_at].cpu().numpy()
    return lay, outs, host, stats.cpu().numpy()


def fields_device(patches, shape, params=None, eng=None, want_stages=False):
    """The smoothed block vectors of every pair of ``patches`` (stage-level device patches:
    ``engine.DevicePatch``) in a mosaic of ``shape``: ``(pairs, fields)`` with ``pairs`` as
    ``pairs_for`` returns them and ``fields[q]`` int16 [nby][nbx][2] = (dx, dy) per level-0 block
    of pair q, ``g_i(s) ~ g_j(s + F)``.  With ``want_stages`` third a dict: ``pyramid`` {(camera,
    level): uint16 grey | valid << 8 over the camera's box}, ``boxes`` {(camera, level): (y0, x0)
    of that array in level samples} and ``vectors`` {(pair, level): int16 [nby][nbx][4] = (dx, dy,
    known, 0)}."""
    params = params or FlowParams()
    lay, _, host, _ = _run(patches, shape, params, eng, False, want_stages)
    fields = [lay.field_of(host, q).copy() for q in range(len(lay.pairs))]
    if not want_stages:
        return lay.pairs, fields
    return lay.pairs, fields, _stages_of(lay, host)


def _stages_of(lay, host):
    return {"pyramid": {k: lay.level_of(host, *k).copy() for k in lay.gv},
            "boxes": {k: v[3:5] for k, v in lay.gv.items()},
            "vectors": {k: lay.vectors_of(host, *k).copy() for k in lay.vec}}


def statistics(lay, host, counts, params):
    """What a run logs: pairs, blocks and the known ones, the median and the largest smoothed
    vector length, the known blocks at the reach, pixels moved and valid."""
    known = np.concatenate([lay.vectors_of(host, q, 0)[..., 2].ravel() for q in range(len(lay.pairs))]
                           or [np.zeros(0, np.int16)]) != 0
    vec = np.concatenate([lay.vectors_of(host, q, 0)[..., :2].reshape(-1, 2) for q in range(len(lay.pairs))]
                         or [np.zeros((0, 2), np.int16)]).astype(np.int64)
    reaches = np.concatenate([np.full(lay.vec[q, 0][1] * lay.vec[q, 0][2], 2 ** (p[2] + 1) - 1)
                              for q, p in enumerate(lay.pairs)] or [np.zeros(0, np.int64)])
    smooth = np.concatenate([lay.field_of(host, q).reshape(-1, 2) for q in range(len(lay.pairs))]
                            or [np.zeros((0, 2), np.int16)]).astype(np.float64)
    length = np.hypot(smooth[:, 0], smooth[:, 1])
    at_reach = known & (np.abs(vec).max(axis=1, initial=0) >= reaches) if len(vec) else known
    return {"pairs": len(lay.pairs), "blocks": int(known.size), "known": int(known.sum()),
            "median": float(np.median(length[known])) if known.any() else 0.0,
            "largest": float(length.max()) if length.size else 0.0,
            "at_reach": int(at_reach.sum()), "moved": int(counts[0]), "valid": int(counts[1]),
            "reach": params.reach}


def align_device(patches, shape, params=None, eng=None, want_stages=False):
    """Aligns stage-level device patches locally in ONE native call and returns ``(aligned,
    statistics)``: every patch that has a pair partner as a copy with new ``planes`` - its
    ``mask``, ``blurred`` and ``scratch`` are the incoming tensors -, every other patch as the very
    object that came in; the statistics as ``statistics`` returns them (the one wait of the call:
    they are read from the device).  With ``want_stages`` third the stages of ``fields_device``
    plus ``fields`` and ``pairs``."""
    params = params or FlowParams()
    lay, outs, host, counts = _run(patches, shape, params, eng, True, want_stages)
    aligned = []
    for p, planes in zip(patches, outs):
        if planes is None:
            aligned.append(p)
            continue
        q = copy.copy(p)
        q.planes = planes
        aligned.append(q)
    stats = statistics(lay, host, counts, params) if lay.pairs else \
        {"pairs": 0, "blocks": 0, "known": 0, "median": 0.0, "largest": 0.0, "at_reach": 0,
         "moved": 0, "valid": 0, "reach": params.reach}
    if not want_stages:
        return aligned, stats
    stages = _stages_of(lay, host)
    stages["fields"] = [lay.field_of(host, q).copy() for q in range(len(lay.pairs))]
    stages["pairs"] = lay.pairs
    return aligned, stats, stages


def log_statistics(stats):
    """The run's log line, and the warning when the frames are further apart than the search
    reaches: more than a tenth of the known blocks at the reach."""
    known = max(stats["known"], 1)
    logging.info(f"Local alignment: {stats['pairs']} pairs, {stats['known'] / max(stats['blocks'], 1):.3f} of "
                 f"{stats['blocks']} blocks known, vector length median {stats['median']:.2f} largest "
                 f"{stats['largest']:.2f} px, {stats['moved'] / max(stats['valid'], 1):.4f} of the valid "
                 f"pixels moved")
    if stats["known"] and stats["at_reach"] > stats["known"] / 10:
        logging.warning(f"Local alignment: {stats['at_reach'] / known:.2f} of the known blocks sit at the "
                        f"search's reach of {stats['reach']} px: the frames are further apart than "
                        f"--local-align-levels reaches")
