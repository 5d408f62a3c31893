"""Bracket deghosting on the device (pano_deghost_u8, csrc/deghost.hip) against the contract's
NumPy model (tests/deghost_model.py) on forged stacks (tests/deghost_cases.py): every stage bit
for bit under every parameter set, the applied frames, the deghosted fusion, batches and workspace
state, every refusal, and the bracketed ingest."""
import ctypes as C
import logging
import os

import numpy as np
import pytest

import align_cases
import align_model
import deghost_cases
import deghost_model
from pano360_amd import _lib, align, deghost, fuse

pytestmark = pytest.mark.gpu


def _dev(eng, frames):
    import torch
    return [torch.from_numpy(np.array(f)).to(eng.device) for f in frames]


def _params(case, values=deghost_cases.PARAMS[0]):
    return deghost.DeghostParams(*values, reference=case[4])


def _same_stages(got, want, k):
    for name in ("hists", "ranks", "maps"):
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), (name, np.argwhere(got[name] != want[name])[:4].tolist())
    for name in ("raw", "mask"):                        # (whole words: the padding bits are 0 in both)
        assert got[name].dtype == np.uint32
        for e in range(k):
            differ = np.argwhere(got[name][e] != want[name][e])[:4].tolist()
            assert np.array_equal(got[name][e], want[name][e]), (name, e, differ)


# ------------------------------------------------------- 1. every stage, bit for bit
@pytest.mark.parametrize("case", deghost_cases.CASES, ids=deghost_cases.IDS)
def test_stages_bit_for_bit(eng, case):
    _, h, w, k, r = case
    frames = _dev(eng, deghost_cases.stack_of(case))
    for values in deghost_cases.PARAMS:
        want = deghost_cases.model_of(case, values)
        (counts,), (got,) = deghost.masks_device([frames], _params(case, values), eng, True)
        assert got["raw"].shape == got["mask"].shape == (k, h, (w + 31) // 32)
        _same_stages(got, want, k)
        assert counts.dtype == np.int32 and np.array_equal(counts, want["counts"]), values


# -------------------------------------------------------------------- 2. apply
@pytest.mark.parametrize("case", [c for c in deghost_cases.CASES if c[0] in ("bright", "dark", "identical", "flat")] +
                         [deghost_cases.CASES[5], deghost_cases.CASES[9], deghost_cases.CASES[12]],
                         ids=lambda c: "-".join(map(str, c)))
def test_apply(eng, case):
    import torch
    frames = _dev(eng, deghost_cases.stack_of(case))
    want = deghost_cases.model_of(case)
    (out,), (counts,) = deghost.deghost_device([frames], _params(case), eng)
    assert np.array_equal(counts, want["counts"])
    for e, (frame, got) in enumerate(zip(frames, out)):
        if want["counts"][e] == 0:
            assert got is frame                         # untouched: the tensor that came in
        else:
            assert got is not frame
            assert np.array_equal(got.cpu().numpy(), want["out"][e]), e
    # a pitched source: a rectangle of a larger tensor gives the same bytes
    w = frames[0].shape[1]
    wide = [torch.from_numpy(np.pad(np.array(f), ((0, 0), (3, 7), (0, 0)), constant_values=201)).to(eng.device)
            for f in deghost_cases.stack_of(case)]
    views = [t[:, 3:3 + w] for t in wide]
    assert all(v.stride(0) == 3 * (w + 10) and not v.is_contiguous() for v in views)
    (pitched,), (counts2,) = deghost.deghost_device([views], _params(case), eng)
    assert np.array_equal(counts2, want["counts"])
    for view, a, b, c in zip(views, out, pitched, want["counts"]):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        assert (b is view) == (c == 0)


def test_host_arrays(eng):
    case = ("bright", 67, 129, 3, 1)
    out, counts = deghost.deghost([list(deghost_cases.stack_of(case))])
    want = deghost_cases.model_of(case)
    assert np.array_equal(counts[0], want["counts"]) and want["counts"][0] > 0
    assert all(np.array_equal(a, b) for a, b in zip(out[0], want["out"]))


# ------------------------------------------------------------- 3. the deghosted fusion
def test_bracket_deghosts_before_it_fuses(eng):
    h, w = 150, 270
    gains = deghost_cases.GAINS[1]
    groups = [["a0.png", "a1.png", "a2.png"]]
    moving = deghost_cases.scene(h, w, gains, "bright")
    got = fuse.Bracket(3, deghost=deghost.DeghostParams()).fuse_groups(_dev(eng, moving), groups, eng)
    cleaned, counts = deghost_model.deghost(moving)
    assert counts[0] > 0 and counts[2] > 0
    want = fuse.fuse_device([_dev(eng, cleaned)], None, eng)
    plain = fuse.Bracket(3).fuse_groups(_dev(eng, moving), groups, eng)
    assert np.array_equal(got[0].cpu().numpy(), want[0].cpu().numpy())
    assert not np.array_equal(got[0].cpu().numpy(), plain[0].cpu().numpy())
    # nothing moves: exactly what it fuses to without `deghost`
    static = deghost_cases.scene(h, w, gains)
    a = fuse.Bracket(3, deghost=deghost.DeghostParams()).fuse_groups(_dev(eng, static), groups, eng)
    b = fuse.Bracket(3).fuse_groups(_dev(eng, static), groups, eng)
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy())


def test_align_then_deghost_with_the_same_reference(eng):
    """The planted scene cropped at a planted shift, the LAST exposure the reference of both
    stages: align moves the others onto it, deghost then takes it as the scene."""
    h, w, margin = 150, 270, 8
    full = deghost_cases.scene(h + 2 * margin, w + 2 * margin, deghost_cases.GAINS[2], "dark")
    offsets = [(5, -3), (-4, 2), (0, 0)]                # (dx, dy) of each exposure's crop
    stack = [np.ascontiguousarray(f[margin + dy:margin + dy + h, margin + dx:margin + dx + w])
             for f, (dx, dy) in zip(full, offsets)]
    how = align.AlignParams(reference=2)
    moved, shifts = align_model.align(stack, 2)
    assert shifts.tolist() == [[5, -3], [-4, 2], [0, 0]]
    cleaned, counts = deghost_model.deghost(moved, 2)
    assert counts[0] > 0 and counts[1] > 0
    groups = [["s0.png", "s1.png", "s2.png"]]
    got = fuse.Bracket(3, align=how, deghost=deghost.DeghostParams()).fuse_groups(_dev(eng, stack), groups, eng)
    want = fuse.fuse_device([_dev(eng, cleaned)], None, eng)
    assert np.array_equal(got[0].cpu().numpy(), want[0].cpu().numpy())
    other, _ = deghost_model.deghost(moved, 1)          # (the default reference gives another frame)
    wrong = fuse.fuse_device([_dev(eng, other)], None, eng)
    assert not np.array_equal(got[0].cpu().numpy(), wrong[0].cpu().numpy())


def test_the_shares_are_logged_and_a_large_one_is_warned_of(eng, caplog):
    case = ("bright", 67, 129, 3, 1)
    want = deghost_cases.model_of(case)["counts"] / (67 * 129)
    with caplog.at_level(logging.INFO):
        fuse.Bracket(3, deghost=deghost.DeghostParams()).fuse_groups(_dev(eng, deghost_cases.stack_of(case)),
                                                                   [["p0.png", "p1.png", "p2.png"]], eng)
    text = [r.getMessage() for r in caplog.records]
    assert any("p0.png" in t and str([round(float(v), 4) for v in want]) in t for t in text), text
    assert not any(r.levelno == logging.WARNING for r in caplog.records) and want.max() <= 0.25
    caplog.clear()
    unrelated = align_cases.random_stack(64, 48, 2, 77)
    assert deghost_model.deghost(unrelated)[1][0] > 0.25 * 64 * 48
    with caplog.at_level(logging.INFO):
        fuse.Bracket(2, deghost=deghost.DeghostParams()).fuse_groups(_dev(eng, unrelated), [["q0.png", "q1.png"]], eng)
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 1 and "q0.png" in warned[0] and "--bracket-align" in warned[0], warned


# -------------------------------------------------------------- the C ABI, directly
def _records(eng, stacks, refs, apply=True, stages=False):
    """HOST records of device stacks, with fresh outputs: (records, dsts, counts, keep)."""
    import torch
    records = (_lib.DeghostStack * len(stacks))()
    dsts, counts, keep = [], [], []
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
        c = torch.full((k,), -77, dtype=torch.int32, device=eng.device)
        rec.counts = c.data_ptr()
        if stages:
            m = torch.full((k, h, (w + 31) // 32), -1, dtype=torch.int32, device=eng.device)
            t = torch.full((k, 3, 256), 0x5A, dtype=torch.uint8, device=eng.device)
            rec.mask, rec.maps = m.data_ptr(), t.data_ptr()
            keep.append((m, t))
        dsts.append(out), counts.append(c)
    return records, dsts, counts, keep


def _need(eng, stacks):
    return sum(int(eng.lib.pano_deghost_work_bytes(int(s[0].shape[0]), int(s[0].shape[1]), len(s))) for s in stacks)


# ------------------------------------------------------------- 4. batches and state
def test_batches_and_state(eng):
    import torch
    names = ("blocks-301x517-k3r1", "random-16x16-k2r0", "blocks-17x33-k8r0", "dark-150x270-k3r1",
             "flat-17x33-k2r1", "bright-301x517-k3r1")  # the largest first and last, a small one behind it
    picks = [deghost_cases.CASES[deghost_cases.IDS.index(n)] for n in names]
    assert len({c[3] for c in picks}) == 3 and len({c[1:3] for c in picks}) == 4
    refs = [c[4] for c in picks]
    stacks = [_dev(eng, deghost_cases.stack_of(c)) for c in picks]
    native = _lib.DeghostParams(*deghost_cases.PARAMS[0])
    singles = []
    for case, stack, r in zip(picks, stacks, refs):
        records, dsts, counts, keep = _records(eng, [stack], [r], stages=True)
        need = _need(eng, [stack])
        work = torch.empty(need, dtype=torch.uint8, device=eng.device)
        _lib.check(eng.lib.pano_deghost_u8(eng.ctx(), records, 1, C.byref(native), work.data_ptr(), need), "single")
        singles.append((dsts[0], counts[0].cpu().numpy(), keep[0][0].cpu().numpy(), keep[0][1].cpu().numpy()))
        assert np.array_equal(singles[-1][1], deghost_cases.model_of(case)["counts"])
    need = _need(eng, stacks)
    work = torch.empty(need, dtype=torch.uint8, device=eng.device)
    runs = []
    for fill in (None, None, 0xFF):                     # twice, then on a poisoned workspace
        if fill is not None:
            work.fill_(fill)
        records, dsts, counts, keep = _records(eng, stacks, refs, stages=True)
        _lib.check(eng.lib.pano_deghost_u8(eng.ctx(), records, len(stacks), C.byref(native), work.data_ptr(), need),
                   "batch")
        runs.append((dsts, counts, keep))
    fresh = torch.full((need,), 0xFF, dtype=torch.uint8, device=eng.device)    # a fresh one, poisoned
    records, dsts, counts, keep = _records(eng, stacks, refs, stages=True)
    _lib.check(eng.lib.pano_deghost_u8(eng.ctx(), records, len(stacks), C.byref(native), fresh.data_ptr(), need),
               "fresh")
    runs.append((dsts, counts, keep))
    for i in (0, 1):                                    # a small stack after a large one, where the batch was
        records, dsts, counts, keep = _records(eng, [stacks[i]], [refs[i]], stages=True)
        _lib.check(eng.lib.pano_deghost_u8(eng.ctx(), records, 1, C.byref(native), work.data_ptr(), need), "reuse")
        runs.append((dsts, counts, keep) if i == 0 else ([None] + dsts, [None] + counts, [(None, None)] + keep))
    for dsts, counts, keep in runs:
        for (one_dst, one_count, one_mask, one_maps), dst, count, (mask, maps) in zip(singles, dsts, counts, keep):
            if dst is None:
                continue
            assert np.array_equal(count.cpu().numpy(), one_count)
            assert np.array_equal(mask.cpu().numpy(), one_mask) and np.array_equal(maps.cpu().numpy(), one_maps)
            for a, b in zip(one_dst, dst):
                assert (a is None) == (b is None)
                if a is not None:                       # (a frame with a count of 0 keeps the fill)
                    assert torch.equal(a, b)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_write_nothing(eng):
    import torch
    h, w, k = 20, 36, 3
    frames = _dev(eng, deghost_cases.blocks_stack(h, w, k, 9))
    need = int(eng.lib.pano_deghost_work_bytes(h, w, k))
    arena = torch.zeros(need + 4 * h * w, dtype=torch.uint8, device=eng.device)
    dst = [torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device=eng.device) for _ in range(k)]
    counts = torch.full((k,), -77, dtype=torch.int32, device=eng.device)

    def record(**over):
        rec = _lib.DeghostStack()
        for e, f in enumerate(frames):
            rec.src[e], rec.src_pitch[e] = f.data_ptr(), f.stride(0)
            rec.dst[e], rec.dst_pitch[e] = dst[e].data_ptr(), dst[e].stride(0)
        rec.counts, rec.w, rec.h, rec.k, rec.reference = counts.data_ptr(), w, h, k, 1
        for name, value in over.items():
            if name.endswith("_at0"):
                getattr(rec, name[:-4])[0] = value
            else:
                setattr(rec, name, value)
        return rec

    def call(recs, n=None, params=(3, 8, 1, 3), work=arena.data_ptr(), work_bytes=need, null=()):
        arr = (_lib.DeghostStack * len(recs))(*recs)
        native = _lib.DeghostParams(*params)
        return eng.lib.pano_deghost_u8(eng.ctx(), None if "stacks" in null else arr, len(recs) if n is None else n,
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
        "slack = -1": call([good], params=(-1, 8, 1, 3)),
        "slack = 16": call([good], params=(16, 8, 1, 3)),
        "tol = -1": call([good], params=(3, -1, 1, 3)),
        "tol = 256": call([good], params=(3, 256, 1, 3)),
        "erode = -1": call([good], params=(3, 8, -1, 3)),
        "erode = 4": call([good], params=(3, 8, 4, 3)),
        "dilate = -1": call([good], params=(3, 8, 1, -1)),
        "dilate = 16": call([good], params=(3, 8, 1, 16)),
        "src pitch": call([record(src_pitch_at0=3 * w - 1)]),
        "dst pitch": call([record(dst_pitch_at0=3 * w - 1)]),
        "null src": call([record(src_at0=None)]),
        "null counts": call([record(counts=None)]),
        "small workspace": call([good], work_bytes=need - 1),
        "a workspace for one of two": call([good, good], work_bytes=2 * need - 1),
        "dst is a source": call([record(dst_at0=frames[2].data_ptr())]),
        "dst overlaps a source": call([record(dst_at0=frames[1].data_ptr() + 3 * w * (h - 1))]),
        "dst in the workspace": call([record(dst_at0=arena.data_ptr() + need - 16)]),
        "the second stack is bad": call([good, record(k=1)], work_bytes=2 * need),
    }
    torch.cuda.synchronize()
    assert all(torch.equal(d, torch.full_like(d, 0xA5)) for d in dst)      # nothing was launched
    assert not arena.any() and torch.equal(counts, torch.full_like(counts, -77))
    assert all(status == _lib.EINVAL for status in refused.values()), refused
    # ... and the same record goes through as it is
    _lib.check(call([good]), "pano_deghost_u8")
    (want,), (want_counts,) = deghost.deghost_device([frames], deghost.DeghostParams(reference=1), eng)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and want_counts[1] == 0 and want_counts[0] > 0
    for e in range(k):
        if want_counts[e]:
            assert torch.equal(dst[e], want[e])
        else:
            assert torch.equal(dst[e], torch.full_like(dst[e], 0xA5)) and want[e] is frames[e]


# -------------------------------------------------------------------- 6. ingest
def test_bracketed_ingest_deghosts(eng, tmp_path):
    from PIL import Image

    from pano360_amd import stitcher
    h, w = 67, 129
    stacks = [deghost_cases.scene(h, w, deghost_cases.GAINS[1], "bright"),
              deghost_cases.scene(h, w, deghost_cases.GAINS[0], "dark")]
    names = [f"pos{p}_exp{e}.png" for p in range(2) for e in range(3)]
    for name, f in zip(names, stacks[0] + stacks[1]):
        Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(os.path.join(tmp_path, name))
    args = stitcher.parse_args([str(tmp_path), "--bracket", "3", "--bracket-deghost"])
    got = stitcher.ingest(str(tmp_path), 1, bracket=fuse.from_args(args))
    cleaned = [deghost_model.deghost(s) for s in stacks]
    assert all(c[1][0] > 0 and c[1][2] > 0 for c in cleaned)
    want = fuse.fuse_device([_dev(eng, c[0]) for c in cleaned], None, eng)
    plain = stitcher.ingest(str(tmp_path), 1, bracket=3)
    assert len(got) == 2
    for a, b, c in zip(got, want, plain):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        assert not np.array_equal(a.cpu().numpy(), c.cpu().numpy())


# ------------------------------------------- 7. past 2^22 pixels, and more than one pass
LARGE = (2048, 2100)                # N > 2^22: N 255 is past 32 bits


def test_a_large_frame(eng):
    h, w = LARGE
    rng = np.random.default_rng(88)
    coarse = rng.integers(0, 256, (2, -(-h // 16), -(-w // 16), 3), dtype=np.uint8)
    stack = [np.ascontiguousarray(np.repeat(np.repeat(c, 16, axis=0), 16, axis=1)[:h, :w]) for c in coarse]
    stack[1][:, : w // 2] = stack[0][:, : w // 2]       # (the left half agrees)
    want = deghost_model.stages(stack, 1)
    assert h * w > 2 ** 22 and 0 < want["counts"][0] < h * w // 2 + 16 * h
    (counts,), (got,) = deghost.masks_device([_dev(eng, stack)], deghost.DeghostParams(reference=1), eng, True)
    _same_stages(got, want, 2)
    assert np.array_equal(counts, want["counts"])


def test_more_frames_than_one_pass_takes(eng):
    """33 stacks of 8 exposures are 264 frames: two passes over the kernels."""
    stacks = [deghost_cases.blocks_stack(16, 19, 8, 300 + i) for i in range(33)]
    counts = deghost.masks_device([_dev(eng, s) for s in stacks], None, eng)
    assert len(counts) == 33
    for stack, found in zip(stacks, counts):
        assert np.array_equal(found, deghost_model.deghost(stack)[1])
