"""Exposure fusion on the device (pano_fuse_u8, csrc/fuse.hip) against the contract's NumPy model
(tests/fuse_model.py) on forged stacks (tests/fuse_cases.py): the raw weights within the derived
float32 bound of a float64 evaluation, everything after them bit for bit, the identity, batches
and workspace reuse, every refusal, and the bracketed ingest."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

import fuse_cases
import fuse_model
from pano360_amd import _lib, fuse

pytestmark = pytest.mark.gpu

RAW_BOUND = 2e-5                    # derived in fuse_model's docstring


def _dev(eng, frames):
    import torch
    return [torch.from_numpy(np.array(f)).to(eng.device) for f in frames]


def _run(eng, frames, params=None, want_stages=True):
    """One stack through fuse_device: (dst, raw [k][h][w], fused_f32) as NumPy arrays."""
    res = fuse.fuse_device([_dev(eng, frames)], params, eng, want_stages)
    if not want_stages:
        return res[0].cpu().numpy()
    (out,), ((raw, fused),) = res
    return out.cpu().numpy(), raw.cpu().numpy(), fused.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _truth(case, exponents):
    """Stage A of a case in float64, made once."""
    return np.stack([fuse_model.raw_weights(f, np.float64, exponents) for f in fuse_cases.stack_of(case)])


# ------------------------------------------------------------- 1. raw weights
@pytest.mark.parametrize("exponents,slack", [((1.0, 1.0, 1.0), 1), ((1.0, 1.0, 0.0), 1),
                                             ((0.0, 0.0, 1.0), 1), ((2.0, 1.0, 1.0), 2)],
                         ids=["111", "110", "001", "211"])
@pytest.mark.parametrize("case", fuse_cases.CASES, ids=fuse_cases.IDS)
def test_raw_weights_against_float64(eng, case, exponents, slack):
    frames = fuse_cases.stack_of(case)
    _, raw, _ = _run(eng, frames, fuse.FuseParams(*exponents))
    truth = _truth(case, exponents)
    assert raw.dtype == np.float32 and raw.shape == truth.shape
    assert np.isfinite(raw).all() and (raw >= np.float32(1e-12)).all()
    err = float(np.abs(raw.astype(np.float64) - truth).max())
    print(f"max |dev - f64| = {err:.3g}")
    assert err <= slack * RAW_BOUND


# ------------------------------------ 2. everything after the weights, bit for bit
@pytest.mark.parametrize("n_levels", [None, 0, 1], ids=["default", "L0", "L1"])
@pytest.mark.parametrize("case", fuse_cases.CASES, ids=fuse_cases.IDS)
def test_pyramids_bit_for_bit(eng, case, n_levels):
    frames = fuse_cases.stack_of(case)
    h, w = frames[0].shape[:2]
    params = fuse.FuseParams(n_levels=n_levels)
    if n_levels is not None and n_levels > fuse.levels_for(h, w):
        with pytest.raises(ValueError, match="n_levels"):    # (a frame without that level)
            _run(eng, frames, params)
        return
    dst, raw, fused = _run(eng, frames, params)
    want_f, want_q = fuse_model.fuse_from_raw(frames, raw, n_levels)
    assert fused.dtype == np.float32 and fused.shape == want_f.shape
    diff = fused.view(np.uint32) != want_f.view(np.uint32)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert np.array_equal(dst, want_q)


# ------------------------------------------------------------------ 3. identity
@pytest.mark.parametrize("shape", fuse_cases.SIZES + (fuse_cases.BIG,), ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity(eng, shape):
    frame = fuse_cases.random_stack(shape[0], shape[1], 1, 77)[0]
    assert np.array_equal(_run(eng, [frame, frame], want_stages=False), frame)


# --------------------------------------------------------- 4. batches and state
def test_batches_and_state(eng):
    import torch
    picks = [fuse_cases.CASES[i] for i in (15, 0, 5, 8, 7, 3)]    # 150 x 270 first, mixed sizes and k
    stacks = [fuse_cases.stack_of(c) for c in picks]
    singles = [_run(eng, s) for s in stacks]
    outs, stages = fuse.fuse_device([_dev(eng, s) for s in stacks], None, eng, True)
    again = fuse.fuse_device([_dev(eng, s) for s in stacks], None, eng)
    plain = fuse.fuse_device([_dev(eng, s) for s in stacks], None, eng, False)
    for (dst, raw, fused), out, (b_raw, b_fused), out2, out3 in zip(singles, outs, stages, again, plain):
        assert np.array_equal(out.cpu().numpy(), dst)              # a batch equals single calls
        assert np.array_equal(b_raw.cpu().numpy().view(np.uint32), raw.view(np.uint32))
        assert np.array_equal(b_fused.cpu().numpy().view(np.uint32), fused.view(np.uint32))
        assert np.array_equal(out2.cpu().numpy(), dst)             # a second call, the same bytes
        assert np.array_equal(out3.cpu().numpy(), dst)             # without the stage outputs
    # a large stack, then a small one through the same workspace: no level reads stale data
    big, small = stacks[0], stacks[2]
    pair = fuse.fuse_device([_dev(eng, big), _dev(eng, small)], None, eng)
    assert np.array_equal(pair[1].cpu().numpy(), singles[2][0])
    assert np.array_equal(pair[0].cpu().numpy(), singles[0][0])
    # a pitched input: a column slice of a wider tensor is passed by its pitch
    frames = stacks[2]
    h, w = frames[0].shape[:2]
    wide = [torch.from_numpy(np.pad(np.array(f), ((0, 0), (3, 7), (0, 0)), constant_values=201)).to(eng.device)
            for f in frames]
    views = [t[:, 3:3 + w] for t in wide]
    assert all(v.stride(0) == 3 * (w + 10) and not v.is_contiguous() for v in views)
    assert _lib.rgb_on_device(views[0], eng) is views[0]
    pitched = fuse.fuse_device([views], None, eng)[0]
    assert np.array_equal(pitched.cpu().numpy(), singles[2][0])


# ------------------------------------------------------------------ 5. refusals
def test_refusals_leave_dst_untouched(eng):
    import torch
    h, w, k = 12, 20, 3
    frames = _dev(eng, fuse_cases.random_stack(h, w, k, 9))
    pattern = torch.full((h, w, 3), 0xA5, dtype=torch.uint8, device=eng.device)
    dst = pattern.clone()
    need = int(eng.lib.pano_fuse_work_bytes(h, w, k))
    arena = torch.zeros(need + 4 * h * w, dtype=torch.uint8, device=eng.device)
    levels = fuse.levels_for(h, w)

    def record(**over):
        rec = _lib.FuseStack()
        for e, f in enumerate(frames):
            rec.src[e], rec.src_pitch[e] = f.data_ptr(), f.stride(0)
        rec.dst, rec.dst_pitch, rec.w, rec.h, rec.k = dst.data_ptr(), dst.stride(0), w, h, k
        for name, value in over.items():
            if name.startswith("src"):
                getattr(rec, name.split("_at")[0])[1] = value
            else:
                setattr(rec, name, value)
        return rec

    def call(recs, n=None, params=(1.0, 1.0, 1.0, -1), work=arena.data_ptr(), work_bytes=need, null=()):
        arr = (_lib.FuseStack * len(recs))(*recs)
        native = _lib.FuseParams(*params)
        return eng.lib.pano_fuse_u8(eng.ctx(), None if "stacks" in null else arr, len(recs) if n is None else n,
                                    None if "params" in null else C.byref(native),
                                    None if "work" in null else work, work_bytes)

    good = record()
    refused = {
        "null stacks": call([good], null=("stacks",)),
        "null params": call([good], null=("params",)),
        "null work": call([good], null=("work",)),
        "n = 0": call([good], n=0),
        "k = 1": call([record(k=1)]),
        "k = 9": call([record(k=9)]),
        "w = 0": call([record(w=0)]),
        "h = 0": call([record(h=0)]),
        "w = 32768": call([record(w=32768, dst_pitch=3 * 32768)]),
        "h = 32768": call([record(h=32768)]),
        "src pitch": call([record(src_pitch_at1=3 * w - 1)]),
        "dst pitch": call([record(dst_pitch=3 * w - 1)]),
        "null src": call([record(src_at1=None)]),
        "null dst": call([record(dst=None)]),
        "n_levels = -2": call([good], params=(1.0, 1.0, 1.0, -2)),
        "n_levels = L + 1": call([good], params=(1.0, 1.0, 1.0, levels + 1)),
        "negative exponent": call([good], params=(-0.5, 1.0, 1.0, -1)),
        "nan exponent": call([good], params=(1.0, float("nan"), 1.0, -1)),
        "infinite exponent": call([good], params=(1.0, 1.0, float("inf"), -1)),
        "small workspace": call([good], work_bytes=need - 1),
        "dst is a source": call([record(src_at1=dst.data_ptr())]),
        "dst overlaps a source": call([record(src_at1=dst.data_ptr() + 3 * w * (h - 1))]),
        "dst in the workspace": call([record(dst=arena.data_ptr() + need - 16)], work_bytes=need),
        "the second stack is bad": call([good, record(k=1)]),
    }
    torch.cuda.synchronize()
    assert torch.equal(dst, pattern)                    # nothing was launched
    assert not arena.any()
    assert all(status == _lib.EINVAL for status in refused.values()), refused
    # ... and the same record goes through as it is
    _lib.check(call([good]), "pano_fuse_u8")
    want = fuse.fuse_device([frames], None, eng)[0]
    assert torch.equal(dst, want) and not torch.equal(dst, pattern)


# -------------------------------------------------------------------- 6. ingest
def test_bracketed_ingest(eng, tmp_path):
    from PIL import Image

    from pano360_amd import stitcher
    h, w = 24, 40
    names = [f"pos{p}_exp{e}.png" for p in range(2) for e in range(3)]
    images = {name: f for name, f in zip(names, fuse_cases.random_stack(h, w, 6, 31))}
    order = list(names)
    random.Random(4).shuffle(order)
    assert order != sorted(order)
    for name in order:                                  # (created out of order)
        Image.fromarray(images[name]).save(os.path.join(tmp_path, name))
    plain = stitcher.ingest(str(tmp_path), 1, bracket=None)
    listed = [f for f in os.listdir(tmp_path) if f.endswith(".png")]
    assert len(plain) == 6
    decoded = {name: t.cpu().numpy() for name, t in zip(listed, plain)}
    for name in names:                                  # as today: BGR of what was written
        assert np.array_equal(decoded[name], images[name][..., ::-1])
    groups = fuse.group_files(listed, 3)
    assert groups == [names[:3], names[3:]]
    want = fuse.fuse_device([_dev(eng, [decoded[n] for n in g]) for g in groups], None, eng)
    for bracket in (3, fuse.Bracket(3)):
        got = stitcher.ingest(str(tmp_path), 1, bracket=bracket)
        assert len(got) == 2
        for a, b in zip(got, want):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    # other weights reach the kernels
    other = stitcher.ingest(str(tmp_path), 1, bracket=fuse.Bracket(3, fuse.FuseParams(1, 1, 0)))
    assert not np.array_equal(other[0].cpu().numpy(), want[0].cpu().numpy())
    with pytest.raises(ValueError, match="6 images"):
        stitcher.ingest(str(tmp_path), 1, bracket=4)
    # a group whose frames differ in size names its files
    Image.fromarray(np.ascontiguousarray(images[names[4]][:, :30])).save(os.path.join(tmp_path, names[4]))
    with pytest.raises(ValueError, match=names[4]):
        stitcher.ingest(str(tmp_path), 1, bracket=3)
