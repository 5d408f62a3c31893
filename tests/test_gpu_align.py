"""Bracket alignment on the device (pano_align_mtb, csrc/align.hip) against the contract's NumPy
model (tests/align_model.py) on forged stacks (tests/align_cases.py): every stage bit for bit, the
planted shifts, the shifted copies, the aligned fusion, batches and workspace state, every refusal,
and the bracketed ingest."""
import ctypes as C
import os

import numpy as np
import pytest

import align_cases
import align_model
from pano360_amd import _lib, align, fuse

pytestmark = pytest.mark.gpu


def _dev(eng, frames):
    import torch
    return [torch.from_numpy(np.array(f)).to(eng.device) for f in frames]


def _params(case):
    _, h, w, _, r = case
    return align.AlignParams(max_bits=align_cases.max_bits_of(h, w), reference=r)


# ------------------------------------------------------- 1. every stage, bit for bit
@pytest.mark.parametrize("case", align_cases.CASES, ids=align_cases.IDS)
def test_stages_bit_for_bit(eng, case):
    _, h, w, k, r = case
    want = align_cases.model_of(case)
    (shifts,), (got,) = align.shifts_device([_dev(eng, align_cases.stack_of(case))], _params(case), eng, True)
    levels = align_cases.levels_of(h, w)
    assert got["medians"].shape == (k, levels + 1) and got["err"].shape == (k, levels + 1, 9)
    for e in range(k):
        for l in range(levels + 1):
            assert got["grey"][e][l].shape == (h >> l, w >> l)
            assert np.array_equal(got["grey"][e][l], want["grey"][e][l]), ("grey", e, l)
    assert np.array_equal(got["medians"], want["medians"])
    for e in range(k):
        for l in range(levels + 1):
            for name in ("tb", "eb"):                   # (whole words: the padding bits are 0 in both)
                assert got[name][e][l].dtype == np.uint32
                assert np.array_equal(got[name][e][l], want[name][e][l]), (name, e, l)
    assert np.array_equal(got["err"], want["err"]), np.argwhere(got["err"] != want["err"])[:4].tolist()
    assert shifts.dtype == np.int32 and np.array_equal(shifts, want["shifts"])


# ------------------------------------------------------------- 2. the planted shifts
def test_planted_shifts_come_back(eng):
    cases = [c for c in align_cases.CASES if c[0] == "planted"]
    for case in cases:                                  # (each with its own max_bits and reference)
        (shifts,) = align.shifts_device([_dev(eng, align_cases.stack_of(case))], _params(case), eng)
        assert shifts.tolist() == [list(o) for o in align_cases.planted_offsets(case)], case


# -------------------------------------------------------------------- 3. apply
@pytest.mark.parametrize("case", [c for c in align_cases.CASES if c[0] in ("planted", "identical")] +
                         [align_cases.CASES[4], align_cases.CASES[6]], ids=lambda c: "-".join(map(str, c)))
def test_apply(eng, case):
    import torch
    frames = _dev(eng, align_cases.stack_of(case))
    want_shifts = align_cases.model_of(case)["shifts"]
    (aligned,), (shifts,) = align.align_device([frames], _params(case), eng)
    assert np.array_equal(shifts, want_shifts)
    for e, (frame, out) in enumerate(zip(frames, aligned)):
        if not want_shifts[e].any():
            assert out is frame                         # untouched: the tensor that came in
        else:
            assert out is not frame
            want = align_model.apply(align_cases.stack_of(case)[e], int(want_shifts[e][0]), int(want_shifts[e][1]))
            assert np.array_equal(out.cpu().numpy(), want), e
    # a pitched source: a rectangle of a larger tensor gives the same bytes
    h, w = frames[0].shape[:2]
    wide = [torch.from_numpy(np.pad(np.array(f), ((0, 0), (3, 7), (0, 0)), constant_values=201)).to(eng.device)
            for f in align_cases.stack_of(case)]
    views = [t[:, 3:3 + w] for t in wide]
    assert all(v.stride(0) == 3 * (w + 10) and not v.is_contiguous() for v in views)
    (pitched,), (shifts2,) = align.align_device([views], _params(case), eng)
    assert np.array_equal(shifts2, want_shifts)
    for view, a, b, s in zip(views, aligned, pitched, want_shifts):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        assert (b is view) == (not s.any())


# ------------------------------------------------------------- 4. the aligned fusion
def test_bracket_aligns_before_it_fuses(eng):
    case = ("planted", 67, 129, 8, 7)
    stack = align_cases.stack_of(case)[4:]              # (-/0/+ ...: four frames, the reference last)
    how = align.AlignParams(reference=3)
    groups = [[f"a{e}.png" for e in range(4)]]
    got = fuse.Bracket(4, align=how).fuse_groups(_dev(eng, stack), groups, eng)
    model_aligned, model_shifts = align_model.align(stack, 3)
    assert model_shifts.tolist() == [[3, -2], [-1, 0], [1, 0], [0, 0]]
    want = fuse.fuse_device([_dev(eng, model_aligned)], None, eng)
    plain = fuse.Bracket(4).fuse_groups(_dev(eng, stack), groups, eng)
    assert np.array_equal(got[0].cpu().numpy(), want[0].cpu().numpy())
    assert not np.array_equal(got[0].cpu().numpy(), plain[0].cpu().numpy())
    # all shifts zero: exactly what it fuses to without `align`
    same = align_cases.stack_of(("identical", 33, 40, 3, 1))
    groups = [["b0.png", "b1.png", "b2.png"]]
    a = fuse.Bracket(3, align=align.AlignParams()).fuse_groups(_dev(eng, same), groups, eng)
    b = fuse.Bracket(3).fuse_groups(_dev(eng, same), groups, eng)
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy())


def test_a_shift_at_the_limit_is_warned_of(eng, caplog):
    import logging
    case = ("planted", 150, 270, 3, 0)                  # 15 = 2^(3+1) - 1 at max_bits = 3
    with caplog.at_level(logging.INFO):
        fuse.Bracket(3, align=_params(case)).fuse_groups(_dev(eng, align_cases.stack_of(case)),
                                                         [["p0.png", "p1.png", "p2.png"]], eng)
    text = [r.getMessage() for r in caplog.records]
    assert any("p0.png" in t and "(15, -15)" in t for t in text), text
    assert any(r.levelno == logging.WARNING and "limit of 15" in r.getMessage() for r in caplog.records)


# -------------------------------------------------------------- the C ABI, directly
def _records(eng, stacks, refs, apply=True, stages=False):
    """HOST records of device stacks, with fresh outputs: (records, dsts, shifts, keep)."""
    import torch
    records = (_lib.AlignStack * len(stacks))()
    dsts, shifts, keep = [], [], []
    for rec, stack, r in zip(records, stacks, refs):
        h, w, k = int(stack[0].shape[0]), int(stack[0].shape[1]), len(stack)
        rec.w, rec.h, rec.k, rec.reference = w, h, k, r
        out = []
        for e, f in enumerate(stack):
            rec.src[e], rec.src_pitch[e] = f.data_ptr(), f.stride(0)
            if apply and e != r:
                out.append(torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device=eng.device))
                rec.dst[e], rec.dst_pitch[e] = out[-1].data_ptr(), out[-1].stride(0)
            else:
                out.append(None)
        s = torch.full((k, 2), -77, dtype=torch.int32, device=eng.device)
        rec.shifts = s.data_ptr()
        if stages:
            levels = align.levels_for(h, w)
            e = torch.full((k, levels + 1, 9), -1, dtype=torch.int32, device=eng.device)
            rec.errs = e.data_ptr()
            keep.append(e)
        dsts.append(out), shifts.append(s)
    return records, dsts, shifts, keep


def _need(eng, stacks):
    return sum(int(eng.lib.pano_align_work_bytes(int(s[0].shape[0]), int(s[0].shape[1]), len(s))) for s in stacks)


# ------------------------------------------------------------- 5. batches and state
def test_batches_and_state(eng):
    import torch
    picks = [align_cases.CASES[i] for i in (6, 0, 14, 2, 16, 6)]     # 301 x 517 first and last
    assert picks[0][1:3] == align_cases.BIG and len({c[3] for c in picks}) == 3
    refs = [c[4] for c in picks]
    stacks = [_dev(eng, align_cases.stack_of(c)) for c in picks]
    native = _lib.AlignParams(6, 4)
    singles = []
    for stack, r in zip(stacks, refs):
        records, dsts, shifts, errs = _records(eng, [stack], [r], stages=True)
        need = _need(eng, [stack])
        work = torch.empty(need, dtype=torch.uint8, device=eng.device)
        _lib.check(eng.lib.pano_align_mtb(eng.ctx(), records, 1, C.byref(native), work.data_ptr(), need), "single")
        singles.append((dsts[0], shifts[0].cpu().numpy(), errs[0].cpu().numpy()))
    for case, (_, s, _) in zip(picks, singles):
        if align_cases.max_bits_of(case[1], case[2]) == 6:
            assert np.array_equal(s, align_cases.model_of(case)["shifts"])
    need = _need(eng, stacks)
    work = torch.empty(need, dtype=torch.uint8, device=eng.device)
    runs = []
    for fill in (None, None, 0xFF):                     # twice, then on a poisoned workspace
        if fill is not None:
            work.fill_(fill)
        records, dsts, shifts, errs = _records(eng, stacks, refs, stages=True)
        _lib.check(eng.lib.pano_align_mtb(eng.ctx(), records, len(stacks), C.byref(native), work.data_ptr(), need),
                   "batch")
        runs.append((dsts, shifts, errs))
    fresh = torch.full((need,), 0xFF, dtype=torch.uint8, device=eng.device)    # a fresh one, poisoned
    records, dsts, shifts, errs = _records(eng, stacks, refs, stages=True)
    _lib.check(eng.lib.pano_align_mtb(eng.ctx(), records, len(stacks), C.byref(native), fresh.data_ptr(), need),
               "fresh")
    runs.append((dsts, shifts, errs))
    for dsts, shifts, errs in runs:
        for (one_dst, one_shift, one_err), dst, shift, err in zip(singles, dsts, shifts, errs):
            assert np.array_equal(shift.cpu().numpy(), one_shift)
            assert np.array_equal(err.cpu().numpy(), one_err)
            for a, b in zip(one_dst, dst):
                assert (a is None) == (b is None)
                if a is not None:                       # (a frame that did not move keeps the fill)
                    assert torch.equal(a, b)


# ------------------------------------------------------------------ 6. refusals
def test_refusals_write_nothing(eng):
    import torch
    h, w, k = 20, 36, 3
    frames = _dev(eng, align_cases.random_stack(h, w, k, 9))
    need = int(eng.lib.pano_align_work_bytes(h, w, k))
    arena = torch.zeros(need + 4 * h * w, dtype=torch.uint8, device=eng.device)
    dst = [torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device=eng.device) for _ in range(k)]
    shifts = torch.full((k, 2), -77, dtype=torch.int32, device=eng.device)

    def record(**over):
        rec = _lib.AlignStack()
        for e, f in enumerate(frames):
            rec.src[e], rec.src_pitch[e] = f.data_ptr(), f.stride(0)
            rec.dst[e], rec.dst_pitch[e] = dst[e].data_ptr(), dst[e].stride(0)
        rec.shifts, rec.w, rec.h, rec.k, rec.reference = shifts.data_ptr(), w, h, k, 1
        for name, value in over.items():
            if name.endswith("_at0"):
                getattr(rec, name[:-4])[0] = value
            else:
                setattr(rec, name, value)
        return rec

    def call(recs, n=None, params=(6, 4), work=arena.data_ptr(), work_bytes=need, null=()):
        arr = (_lib.AlignStack * len(recs))(*recs)
        native = _lib.AlignParams(*params)
        return eng.lib.pano_align_mtb(eng.ctx(), None if "stacks" in null else arr, len(recs) if n is None else n,
                                      None if "params" in null else C.byref(native),
                                      None if "work" in null else work, work_bytes)

    good = record()
    refused = {
        "null stacks": call([good], null=("stacks",)),
        "null params": call([good], null=("params",)),
        "null work": call([good], null=("work",)),
        "n = 0": call([good], n=0),
        "k = 1": call([record(k=1, reference=0)]),
        "k = 9": call([record(k=9)]),
        "w = 0": call([record(w=0)]),
        "h = 0": call([record(h=0)]),
        "w = 32768": call([record(w=32768)]),
        "h = 32768": call([record(h=32768)]),
        "reference = -1": call([record(reference=-1)]),
        "reference = k": call([record(reference=k)]),
        "max_bits = -1": call([good], params=(-1, 4)),
        "max_bits = 8": call([good], params=(8, 4)),
        "exclude = -1": call([good], params=(6, -1)),
        "exclude = 128": call([good], params=(6, 128)),
        "src pitch": call([record(src_pitch_at0=3 * w - 1)]),
        "dst pitch": call([record(dst_pitch_at0=3 * w - 1)]),
        "null src": call([record(src_at0=None)]),
        "null shifts": call([record(shifts=None)]),
        "small workspace": call([good], work_bytes=need - 1),
        "a workspace for one of two": call([good, good], work_bytes=2 * need - 1),
        "dst is a source": call([record(dst_at0=frames[2].data_ptr())]),
        "dst overlaps a source": call([record(dst_at0=frames[1].data_ptr() + 3 * w * (h - 1))]),
        "dst in the workspace": call([record(dst_at0=arena.data_ptr() + need - 16)]),
        "the second stack is bad": call([good, record(k=1)], work_bytes=2 * need),
    }
    torch.cuda.synchronize()
    assert all(torch.equal(d, torch.full_like(d, 0xA5)) for d in dst)      # nothing was launched
    assert not arena.any() and torch.equal(shifts, torch.full_like(shifts, -77))
    assert all(status == _lib.EINVAL for status in refused.values()), refused
    # ... and the same record goes through as it is
    _lib.check(call([good]), "pano_align_mtb")
    (want,), (want_shifts,) = align.align_device([frames], align.AlignParams(reference=1), eng)
    assert np.array_equal(shifts.cpu().numpy(), want_shifts) and not want_shifts[1].any()
    for e in range(k):
        if want_shifts[e].any():
            assert torch.equal(dst[e], want[e])
        else:
            assert torch.equal(dst[e], torch.full_like(dst[e], 0xA5)) and want[e] is frames[e]


# -------------------------------------------------------------------- 7. ingest
def test_bracketed_ingest_aligns(eng, tmp_path):
    from PIL import Image

    from pano360_amd import stitcher
    case = ("planted", 67, 129, 8, 7)
    frames = align_cases.stack_of(case)
    names = [f"pos{p}_exp{e}.png" for p in range(2) for e in range(3)]
    picks = [frames[3], frames[7], frames[4], frames[0], frames[7], frames[1]]    # the reference in the middle
    for name, f in zip(names, picks):
        Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(os.path.join(tmp_path, name))
    how = align.AlignParams()
    got = stitcher.ingest(str(tmp_path), 1, bracket=fuse.Bracket(3, align=how))
    stacks = [picks[:3], picks[3:]]
    moved = [align_model.align(s) for s in stacks]
    assert [m[1].tolist() for m in moved] == [[[-5, 4], [0, 0], [3, -2]], [[7, -7], [0, 0], [-7, 7]]]
    want = fuse.fuse_device([_dev(eng, m[0]) for m in moved], None, eng)
    plain = stitcher.ingest(str(tmp_path), 1, bracket=3)
    assert len(got) == 2
    for a, b, c in zip(got, want, plain):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        assert not np.array_equal(a.cpu().numpy(), c.cpu().numpy())


# ------------------------------------------- 8. the deepest pyramid, and more than one pass
DEEP = (2048, 2100)                 # L = 7 with max_bits = 7: the levels whose tile part is 4, 2 and 1 pixels


def test_the_deepest_pyramid(eng):
    h, w = DEEP
    stack = align_cases.planted_stack(h, w, [(100, -70)], (1.0, 2.0), True, seed=77, reference=1)
    want = align_model.stages(stack, 1, 7)
    assert align.levels_for(h, w, 7) == 7 and want["shifts"].tolist() == [[100, -70], [0, 0]]
    (shifts,), (got,) = align.shifts_device([_dev(eng, stack)], align.AlignParams(7, reference=1), eng, True)
    assert np.array_equal(shifts, want["shifts"]) and np.array_equal(got["medians"], want["medians"])
    assert np.array_equal(got["err"], want["err"])
    for e in range(2):
        for l in range(8):
            for name in ("grey", "tb", "eb"):
                assert np.array_equal(got[name][e][l], want[name][e][l]), (name, e, l)


def test_more_frames_than_one_pass_takes(eng):
    """33 stacks of 8 exposures are 264 frames: two passes over the kernels."""
    stacks = [align_cases.random_stack(16, 19, 8, 300 + i) for i in range(33)]
    shifts = align.shifts_device([_dev(eng, s) for s in stacks], None, eng)
    assert len(shifts) == 33
    for stack, found in zip(stacks, shifts):
        assert np.array_equal(found, align_model.shifts(stack))
