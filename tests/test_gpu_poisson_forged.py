"""GPU: the Poisson blend (csrc/poisson.hip through blend.poisson_blend_device) on the forged
cases of tests/poisson_cases.py: masks on the stencil's quirks and on the borders of a lane's
pair, a wave's 128 elements and a block's 2048; shapes down to 1 x 2; channels that converge
before the first iteration, in one exact step, or not within the cap; solutions that clip.

The reference is tests/poisson_model.py solved by SciPy's direct solver (poisson_cases.solved).
GUARD and LEFT_OUT are those of tests/test_gpu_poisson.py and mean the same.  Per case:
 (a) the returned float64 solution is within GUARD of the reference's at every pixel and is the
     target, exactly, outside the mask;
 (b) every byte inside the mask is np.clip(sol, 0, 255).astype(uint8) of the solution the same
     call returned, every byte outside is the target's - exact, no pixel left out;
 (c) the bytes equal the reference's at every pixel whose reference solution is farther than
     GUARD from an integer it could cross, and are within one level elsewhere; a "generic" case
     leaves out at most LEFT_OUT of the mask per channel, an "integral" one (solutions integral
     by construction, test_poisson_cases_host.py) any share;
 (d) the final ||r|| / ||b|| is at most 1e-12 and a second run gives the same bits."""
import numpy as np
import pytest

import poisson_cases as pc
import poisson_model as pm
from poisson_cases import GUARD, LEFT_OUT

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def run(eng, src, tgt, mask, **kw):
    """poisson_blend_device on host arrays: (uint8 result [H][W][C], float64 solution
    [C][H][W], iterations, residuals)."""
    import torch
    from pano360_amd import blend
    out, sol, iters, resid = blend.poisson_blend_device(
        torch.from_numpy(np.array(src)).to(eng.device),     # copies: the cases are read-only
        torch.from_numpy(np.array(tgt)).to(eng.device),
        torch.from_numpy(np.array(mask)).to(eng.device), eng, want_solution=True,
        **kw)
    return out.cpu().numpy(), sol.cpu().numpy(), iters.copy(), resid.copy()


def run_case(eng, name, **kw):
    case = pc.CASES[name]
    return run(eng, case.src, case.tgt, case.mask, **kw)


def check(name, got, case=None, ref=None):
    """(a), (b), (c) and the residual of (d); prints the figures before it asserts."""
    case = case or pc.CASES[name]
    ref_sol, ref_u8 = ref or pc.solved(name)
    got_u8, got_sol, iters, resid = got
    inside = case.mask
    C = case.tgt.shape[2]
    planes = case.tgt.transpose(2, 0, 1)
    assert got_sol.shape == ref_sol.shape and got_u8.shape == case.tgt.shape
    dev = np.abs(got_sol - ref_sol).reshape(C, -1).max(axis=1)
    print(f"{name} [{case.cls}, {inside.sum()} mask pixels]: iterations {iters.tolist()}, "
          f"residuals {resid.tolist()}, max |sol - ref| {dev.max():.3e}")
    assert np.isfinite(got_sol).all()
    assert (dev <= GUARD).all(), (name, dev)                                        # (a)
    assert np.array_equal(got_sol[:, ~inside], planes[:, ~inside].astype(np.float64)), name
    want = np.clip(got_sol, 0, 255).astype(np.uint8).transpose(1, 2, 0)             # (b)
    assert np.array_equal(got_u8[inside], want[inside]), name
    assert np.array_equal(got_u8[~inside], case.tgt[~inside]), name
    for c in range(C):                                                              # (c)
        safe = pm.safe_pixels(ref_sol[c][inside], GUARD)
        share = np.mean(~safe)
        a, b = got_u8[..., c][inside].astype(int), ref_u8[..., c][inside].astype(int)
        wrong, off = int((a[safe] != b[safe]).sum()), int(np.abs(a - b).max())
        print(f"  channel {c}: left out {100 * share:.4f} %, {wrong} safe pixels differ, "
              f"max byte gap {off}")
        assert wrong == 0 and off <= 1, (name, c, wrong, off)
        if case.cls == "generic" or (name == "same_channel" and c in pc.SAME_GENERIC):
            assert share <= LEFT_OUT, (name, c, share)
    assert (resid <= RTOL).all() and (resid >= 0).all(), (name, resid)              # (d)
    assert len(iters) == len(resid) == C


def same_bits(a, b):
    return (np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
            and np.array_equal(a[2], b[2]) and a[3].tobytes() == b[3].tobytes())


def channel_alone(case, c):
    return pc.Case(np.ascontiguousarray(case.src[..., c:c + 1]),
                   np.ascontiguousarray(case.tgt[..., c:c + 1]), case.mask, case.cls)


# ---- 1. every case against the direct solve ---------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_case_against_the_direct_solve(eng, name):
    first = run_case(eng, name)
    check(name, first)
    assert same_bits(first, run_case(eng, name)), name


# ---- 2. solver states -------------------------------------------------------------------------
def test_channel_converged_before_the_first_iteration_stays_frozen(eng):
    case = pc.CASES["same_channel"]
    got_u8, got_sol, iters, resid = run_case(eng, "same_channel")
    print("iterations", iters.tolist(), "residuals", resid.tolist())
    assert iters[1] == 0 and resid[1] == 0.0
    assert np.array_equal(got_u8[..., 1], case.tgt[..., 1])
    assert np.array_equal(got_sol[1], case.tgt[..., 1].astype(np.float64))
    assert (iters[[0, 2, 3]] >= 1).all() and (resid[[0, 2, 3]] > 0).all()
    for c in (0, 2, 3):
        assert not np.array_equal(got_u8[..., c][case.mask], case.tgt[..., c][case.mask])


@pytest.mark.parametrize("name", ["one_pixel", "isolated", "odd_flat", "even_flat", "single_0",
                                  "single_2047", "single_2048", "single_8776"])
def test_one_exact_step(eng, name):
    """On an isolated mask A is 4 I: alpha = 1/4 exactly (r0 holds small integers, so both dot
    products are exact), s = r - alpha v = 0, t = 0, omega = 0, beta NaN - and the channel has
    converged with r = 0, which the verdict must see before the NaN."""
    got = run_case(eng, name)
    print(name, "iterations", got[2].tolist(), "residuals", got[3].tolist())
    assert (got[2] == 1).all(), got[2]
    assert (got[3] == 0.0).all(), got[3]
    case = pc.CASES[name]
    ref_sol, _ = pc.solved(name)
    # x0 + r0 / 4 in float64 is the exact k / 4
    assert np.array_equal(got[1][:, case.mask], np.rint(ref_sol[:, case.mask] * 4) / 4)


def test_zero_right_hand_side(eng):
    case = pc.CASES["zero"]
    got_u8, got_sol, iters, resid = run_case(eng, "zero")
    assert (iters == 0).all() and (resid == 0.0).all()
    assert np.array_equal(got_u8, case.tgt) and not got_sol.any()


# ---- 3. channels are independent, bit for bit -------------------------------------------------
@pytest.mark.parametrize("name", ["same_channel", "clip"])
def test_channel_among_others_has_the_bits_it_has_alone(eng, name):
    case = pc.CASES[name]
    u8, sol, iters, resid = run_case(eng, name)
    print(name, "iterations", iters.tolist())
    for c in range(case.src.shape[2]):
        one = channel_alone(case, c)
        a_u8, a_sol, a_iters, a_resid = run(eng, one.src, one.tgt, one.mask)
        assert a_sol[0].tobytes() == sol[c].tobytes(), (name, c)
        assert a_iters[0] == iters[c] and a_resid[0] == resid[c], (name, c)
        assert np.array_equal(a_u8[..., 0], u8[..., c]), (name, c)


# ---- 4. the iteration cap and the chunks ------------------------------------------------------
def test_iteration_cap_in_and_between_chunks(eng):
    """max_iters = N ends in a partial chunk (or, at a multiple of 32, in a whole one) and gives
    the bits of the default run; N - 1 is the ordinary error return and leaves the target."""
    import torch
    from pano360_amd import _lib, blend
    counts = {}
    for name in ("wrap", "full_33x47", "clip"):
        one = channel_alone(pc.CASES[name], 0)
        ref = tuple(a[:1] if k == 0 else a[..., :1] for k, a in enumerate(pc.solved(name)))
        default = run(eng, one.src, one.tgt, one.mask)
        N = counts[name] = int(default[2][0])
        check(name + "[0]", default, one, ref)
        exact = run(eng, one.src, one.tgt, one.mask, max_iters=N)
        assert exact[2][0] == N and same_bits(default, exact), name
        dev_tgt = torch.from_numpy(one.tgt.copy()).to(eng.device)
        with pytest.raises(_lib.PanoError, match=f"not converged after {N - 1} iterations"):
            blend.poisson_blend_device(torch.from_numpy(one.src.copy()).to(eng.device), dev_tgt,
                                       torch.from_numpy(one.mask.copy()).to(eng.device), eng,
                                       max_iters=N - 1)
        assert np.array_equal(dev_tgt.cpu().numpy(), one.tgt), name
        assert same_bits(default, run(eng, one.src, one.tgt, one.mask)), name
    print("iterations", counts)
    assert 1 < counts["wrap"] < 32, counts                 # within the first chunk
    assert counts["full_33x47"] > 96, counts               # more than three chunks
    assert counts["wrap"] % 32 and (counts["full_33x47"] % 32 or counts["clip"] % 32), counts


# ---- 5. a non-contiguous source ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["wrap", "clip"])
def test_non_contiguous_source(eng, name):
    import torch
    from pano360_amd import blend
    case = pc.CASES[name]
    H, W, C = case.src.shape
    wide = np.full((H, W + 9, C), 77, np.uint8)
    wide[:, 4:4 + W] = case.src
    view = torch.from_numpy(wide).to(eng.device)[:, 4:4 + W]
    assert not view.is_contiguous()
    out, sol, iters, resid = blend.poisson_blend_device(
        view, torch.from_numpy(case.tgt.copy()).to(eng.device),
        torch.from_numpy(case.mask.copy()).to(eng.device), eng, want_solution=True)
    got = (out.cpu().numpy(), sol.cpu().numpy(), iters, resid)
    assert same_bits(got, run_case(eng, name))
    assert np.array_equal(view.cpu().numpy(), case.src)
    check(name, got)


# ---- 6. state across calls on one fresh engine ------------------------------------------------
def test_state_across_calls_on_a_fresh_engine(eng):
    """The solver's scratch and the channels' records are the context's: a one-pixel blend runs
    in the front of buffers that held 4095 unknowns of three channels and then four channels
    of which one never started."""
    from pano360_amd import engine
    use = engine.Engine(eng.device)
    order = ("one_pixel", "full_45x91", "one_pixel", "same_channel", "one_pixel")
    got = [run_case(use, name) for name in order]
    for name, g in zip(order, got):
        check(name, g)
    assert same_bits(got[0], got[2]) and same_bits(got[0], got[4])
    assert (got[0][2] == 1).all()
