"""GPU: the Poisson blend (csrc/poisson.hip through blend.poisson_blend and
blend.poisson_blend_device).

The device solves the reference's linear system by a float64 BiCGStab iteration; the reference
factorises it.  What is compared is therefore the float64 solution, and the bytes where a
truncation cannot flip:

GUARD = 1e-4 grey levels.  The solution is consumed by a truncation to 8 bits, so 1e-4 of a
level is invisible; it is about 300 times what a float64 BiCGStab left against the direct solve
on the CPU (3e-7) and far below what a float32 Krylov solve reaches.  The device solution must
be within GUARD of the reference's recorded ``sol`` at every mask pixel; the uint8 result must
equal the reference's at every mask pixel whose ``sol`` is farther than GUARD from an integer
(beyond the clip range: from 0 or 255), the pixels left out may be at most LEFT_OUT = 0.2 % of
the mask per channel and must still be within one level; outside the mask the bytes are the
target's.  Fixtures: tests/golden/poisson_*.npz (tools/gen_poisson_golden.py); the full-size
case is checked against tests/poisson_model.py solved by SciPy's direct solver here."""
import glob
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import poisson_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 1e-4
LEFT_OUT = 0.002
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "poisson_*.npz")))


def blend_on_device(eng, src, tgt, mask, **kw):
    """poisson_blend_device on host arrays: (uint8 result [H][W][C], float64 solution
    [C][H][W], iterations, residuals)."""
    import torch
    from pano360_amd import blend
    out, sol, iters, resid = blend.poisson_blend_device(
        torch.from_numpy(src).to(eng.device), torch.from_numpy(tgt.copy()).to(eng.device),
        torch.from_numpy(np.ascontiguousarray(mask)).to(eng.device), eng, want_solution=True,
        **kw)
    return out.cpu().numpy(), sol.cpu().numpy(), iters, resid


def check_against(label, got_u8, got_sol, tgt, mask, ref_sol, ref_u8):
    """The two criteria of the module docstring.  ref_sol: [C][H][W]; prints the figures before
    it asserts."""
    inside = mask != 0
    assert np.array_equal(got_u8[~inside], tgt[~inside]), "bytes outside the mask changed"
    for c in range(ref_sol.shape[0]):
        dev = np.abs(got_sol[c][inside] - ref_sol[c][inside]).max()
        safe = pm.safe_pixels(ref_sol[c][inside], GUARD)
        share = np.mean(~safe)
        a, b = got_u8[..., c][inside].astype(int), ref_u8[..., c][inside].astype(int)
        wrong = int((a[safe] != b[safe]).sum())
        off = int(np.abs(a - b).max())
        print(f"{label} channel {c}: max |sol - ref| {dev:.3e}, left out {100 * share:.4f} % "
              f"of {inside.sum()} mask pixels, {wrong} safe pixels differ, max byte gap {off}")
        assert dev <= GUARD, (label, c, dev)
        assert share <= LEFT_OUT, (label, c, share)
        assert wrong == 0, (label, c, wrong)
        assert off <= 1, (label, c, off)


@pytest.fixture(scope="module", params=FIXTURES, ids=lambda p: os.path.basename(p)[8:-4])
def golden(request):
    return dict(np.load(request.param))


def full_solution(g):
    """The fixture's sol (stored at the mask pixels) on the grid; the target elsewhere."""
    inside = g["mask"] != 0
    sol = g["tgt"].transpose(2, 0, 1).astype(np.float64)
    for c in range(sol.shape[0]):
        sol[c][inside] = g["sol"][c]
    return sol


def test_fixtures_present():
    assert len(FIXTURES) == 3, FIXTURES


def test_solution_and_bytes_against_the_reference(eng, golden):
    """Tests 5 and 6 of the issue: every fixture case and channel."""
    got_u8, got_sol, iters, resid = blend_on_device(eng, golden["src"], golden["tgt"],
                                                    golden["mask"])
    print("iterations", iters.tolist(), "residuals", resid.tolist())
    assert (iters > 0).all() and (resid <= 1e-12).all()
    check_against("fixture", got_u8, got_sol, golden["tgt"], golden["mask"],
                  full_solution(golden), golden["result"])


def test_public_call_matches_the_reference_bytes(eng, golden):
    """blend.poisson_blend itself (through the top-level shim) on the fixture's host arrays."""
    import blend
    tgt = golden["tgt"].copy()
    out = blend.poisson_blend(golden["src"], tgt, golden["mask"])
    assert out is tgt
    inside = golden["mask"] != 0
    assert np.array_equal(out[~inside], golden["tgt"][~inside])
    for c in range(out.shape[2]):
        safe = pm.safe_pixels(golden["sol"][c], GUARD)
        assert np.array_equal(out[..., c][inside][safe], golden["result"][..., c][inside][safe])


def small_case(C=3, H=40, W=52, seed=7):
    src, tgt = pm.textured(H, W, C, seed), pm.textured(H, W, C, seed + 1)
    y, x = np.mgrid[:H, :W]
    mask = ((x - 0.7 * W) / (0.4 * W)) ** 2 + ((y - 0.5 * H) / (0.35 * H)) ** 2 <= 1.0
    return src, tgt, mask


def test_contract_target_mutated_source_and_mask_untouched(eng):
    from pano360_amd import blend
    src, tgt, mask = small_case()
    src0, tgt0 = src.copy(), tgt.copy()
    results = []
    for m in (mask, mask.astype(np.uint8) * 255, mask.astype(np.float64) * 0.25,
              mask.astype(np.float32) * -3.0, mask.astype(np.int32) * 7):
        m0 = m.copy()
        target = tgt0.copy()
        out = blend.poisson_blend(src, target, m)
        assert out is target
        assert np.array_equal(src, src0) and np.array_equal(m, m0) and m.dtype == m0.dtype
        assert np.array_equal(out[~mask], tgt0[~mask])
        assert not np.array_equal(out[mask], tgt0[mask])
        results.append(out)
    for other in results[1:]:
        assert np.array_equal(other, results[0])
    _, ref_u8 = pm.solve(src0, tgt0, mask)
    assert np.abs(results[0].astype(int) - ref_u8.astype(int)).max() <= 1


def test_contract_empty_mask_returns_the_target_unchanged(eng):
    from pano360_amd import blend
    src, tgt, mask = small_case()
    target = tgt.copy()
    out = blend.poisson_blend(src, target, np.zeros_like(mask))
    assert out is target and np.array_equal(out, tgt)
    got_u8, got_sol, iters, _ = blend_on_device(eng, src, tgt, np.zeros(mask.shape, np.uint8))
    assert np.array_equal(got_u8, tgt) and (iters == 0).all()
    assert np.array_equal(got_sol, tgt.transpose(2, 0, 1).astype(np.float64))


@pytest.mark.parametrize("C", [1, 3, 4])
def test_contract_channel_counts(eng, C):
    src, tgt, mask = small_case(C=C, seed=20 + C)
    got_u8, got_sol, iters, _ = blend_on_device(eng, src, tgt, mask)
    ref_sol, ref_u8 = pm.solve(src, tgt, mask)
    assert got_u8.shape == tgt.shape and got_sol.shape == ref_sol.shape and len(iters) == C
    assert np.abs(got_sol - ref_sol).max() <= GUARD
    inside = mask != 0
    for c in range(C):
        safe = pm.safe_pixels(ref_sol[c][inside], GUARD)
        assert np.array_equal(got_u8[..., c][inside][safe], ref_u8[..., c][inside][safe])


def test_contract_out_of_scope_inputs_raise(eng):
    from pano360_amd import blend
    src, tgt, mask = small_case()
    with pytest.raises(NotImplementedError):
        blend.poisson_blend(src.astype(np.float32), tgt.astype(np.float32), mask)
    with pytest.raises(NotImplementedError):
        blend.poisson_blend(src.astype(np.uint16), tgt.astype(np.uint16), mask)
    with pytest.raises(ValueError):
        blend.poisson_blend(src, tgt[:-1], mask)
    with pytest.raises(ValueError):
        blend.poisson_blend(src, tgt, mask[:, :-1])
    with pytest.raises(ValueError):
        blend.poisson_blend(np.dstack([src, src]), np.dstack([tgt, tgt]), mask)
    with pytest.raises(ValueError):
        blend.poisson_blend(src[:, :1], tgt[:, :1].copy(), mask[:, :1])
    assert np.array_equal(tgt, small_case()[1])


def test_same_blend_twice_gives_the_same_bits(eng, golden):
    first = blend_on_device(eng, golden["src"], golden["tgt"], golden["mask"])
    again = blend_on_device(eng, golden["src"], golden["tgt"], golden["mask"])
    assert first[1].tobytes() == again[1].tobytes()
    assert np.array_equal(first[0], again[0])
    assert np.array_equal(first[2], again[2]) and first[3].tobytes() == again[3].tobytes()


def test_small_large_small_on_one_engine(eng):
    """The solver's scratch is the context's: it grows for the larger blend and the smaller one
    then runs in the front of a buffer that holds the larger one's vectors."""
    small = small_case(C=3, H=33, W=47, seed=31)          # odd sizes: the padded tail is in use
    g = dict(np.load(FIXTURES[-1]))
    src_l, tgt_l = pm.textured(310, 270, 4, 41), pm.textured(310, 270, 4, 42)
    mask_l = pm.seam_mask(310, 270, 5)
    first = blend_on_device(eng, *small)
    large = blend_on_device(eng, src_l, tgt_l, mask_l)
    again = blend_on_device(eng, *small)
    assert first[1].tobytes() == again[1].tobytes() and np.array_equal(first[0], again[0])
    assert np.array_equal(first[2], again[2])
    # a fixture in between and after: still the reference's answer
    got = blend_on_device(eng, g["src"], g["tgt"], g["mask"])
    check_against("after growth", got[0], got[1], g["tgt"], g["mask"], full_solution(g),
                  g["result"])
    large_again = blend_on_device(eng, src_l, tgt_l, mask_l)
    assert large[1].tobytes() == large_again[1].tobytes()
    ref_sol, _ = pm.solve(*small)
    assert np.abs(first[1] - ref_sol).max() <= GUARD


def test_full_size_against_the_direct_solve(eng):
    """An overlap-sized blend without a fixture: 720 x 652 x 3, a seam-like mask over about half
    the pixels that touches the top, the bottom and the right edge, against poisson_model
    solved by SciPy's direct solver (one factorisation, three right-hand sides), with the same
    two criteria as the fixtures.  It is larger than 540 x 488 because the CPU solve leaves the
    room: building, factorising and solving took 3.4 s on the development machine's CPU and
    1.0 s on the GPU machine's (540 x 488: 1.7 s for one channel with a factorisation per
    channel).  At this size BiCGStab takes 1200 to 1450 iterations per channel - the same
    recurrence in NumPy took 1305 to 1352 - which is some forty chunked convergence readbacks,
    with the channels stopping in different chunks."""
    H, W, C = 720, 652, 3
    src, tgt = pm.textured(H, W, C, 51), pm.textured(H, W, C, 52)
    mask = pm.seam_mask(H, W, 9)
    assert mask[0].any() and mask[-1].any() and mask[:, -1].all() and 0.4 < mask.mean() < 0.6
    t0 = time.time()
    ref_sol, ref_u8 = pm.solve(src, tgt, mask)
    print(f"direct solve on the CPU: {time.time() - t0:.1f} s")
    got_u8, got_sol, iters, resid = blend_on_device(eng, src, tgt, mask)
    print("iterations", iters.tolist(), "residuals", resid.tolist())
    assert (iters >= 1000).all(), iters
    check_against("full size", got_u8, got_sol, tgt, mask, ref_sol, ref_u8)


def test_failure_is_loud_and_leaves_the_target(eng):
    import torch
    from pano360_amd import _lib, blend
    src, tgt, mask = small_case()
    dev_tgt = torch.from_numpy(tgt.copy()).to(eng.device)
    with pytest.raises(_lib.PanoError, match="not converged after 5 iterations"):
        blend.poisson_blend_device(torch.from_numpy(src).to(eng.device), dev_tgt,
                                   torch.from_numpy(mask).to(eng.device), eng, max_iters=5)
    assert np.array_equal(dev_tgt.cpu().numpy(), tgt)
    # ... and the engine is fine afterwards
    got_u8, got_sol, _, _ = blend_on_device(eng, src, tgt, mask)
    assert np.abs(got_sol - pm.solve(src, tgt, mask)[0]).max() <= GUARD
