"""GPU: pano_ba_residuals and pano_ba_normal (csrc/bundle.hip) through their native entries on a
forged pair table (ba_model.forged_system): pairs of 0 to 1000 matches on both sides of the
wave's 64 and the block's 256 lanes, cameras left out so that slot[c] != c, a camera in six
pairs, one pair of cameras twice, regions in a shuffled order between rows of NaN, r at another
camera state than J.

include/pano360.h fixes the order of every addition ("the same input gives the same bits"), so
the kernels are compared BIT FOR BIT with ba_model's ordered restatement (ssq_ordered,
pair_sums_ordered, assemble_ordered), and, as a check that shares no summation with either,
with ba_model.normal_equations / pair_ssq in the scaled measures and the 1e-12 bound of
test_gpu_bundle.py's test_kernels_match_reference.  Outputs are prefilled with NaN."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_model as bm  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class _Forged:
    """The forged system on the device and one run of both entries over it."""

    def __init__(self, eng):
        import torch
        self.eng, self.torch = eng, torch
        self.f = f = bm.forged_system()
        self.n_pairs, self.n_active = len(f["pairs"]), int(f["n_active"])
        self.host = {"rows": f["rows"], "pairs": f["pairs"], "slot": f["slot"],
                     "jtab": f["jtab"], "hom_r": f["hom_r"]}
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(eng.device)
                    for k, v in self.host.items()}
        assert self.dev["pairs"].dtype == torch.int32 and self.dev["slot"].dtype == torch.int32
        first, count = f["pairs"][:, 2].astype(np.int64), f["pairs"][:, 3].astype(np.int64)
        assert first.min() >= 0 and (first + count).max() <= len(f["rows"])
        assert 0 <= f["pairs"][:, :2].min() and f["pairs"][:, :2].max() < len(f["slot"])

    def nan(self, *shape):
        return self.torch.full(shape, float("nan"), dtype=self.torch.float64,
                               device=self.eng.device)

    def normal(self, n_pairs=None, n_active=None, slot=True, inputs=True, lam=bm.LAMBDA,
               refused=False):
        """pano_ba_normal into NaN-filled buffers: (jtj, jtr, work [n_pairs][90]) on the host.
        ``refused``: the call is expected to fail, and what it left is returned all the same."""
        from pano360_amd import _lib, engine
        n_pairs = self.n_pairs if n_pairs is None else n_pairs
        n_active = self.n_active if n_active is None else n_active
        d, ptr = self.dev, engine._ptr
        n = 6 * max(n_active, 1)
        work_bytes = int(self.eng.lib.pano_ba_work_bytes(max(n_pairs, 0)))
        assert work_bytes >= 8 * 90 * max(n_pairs, 0)
        work = self.nan(max(work_bytes, 8 * 90 * self.n_pairs) // 8 + 1)
        jtj, jtr = self.nan(n, n), self.nan(n)
        ins = [ptr(d[k]) if inputs else None for k in ("rows", "pairs", "jtab", "hom_r")]
        status = self.eng.lib.pano_ba_normal(
            self.eng.ctx(), ins[0], ins[1], n_pairs, ptr(d["slot"]) if slot else None, n_active,
            ins[2], ins[3], C.c_double(lam), ptr(work) if inputs else None, ptr(jtj), ptr(jtr))
        out = (jtj.cpu().numpy(), jtr.cpu().numpy(),
               work.cpu().numpy()[:90 * max(n_pairs, 0)].reshape(-1, 90))
        if refused:
            assert status != 0
        else:
            _lib.check(status, "pano_ba_normal")
        return out

    def residuals(self, hom, n_pairs=None):
        from pano360_amd import _lib, engine
        n_pairs = self.n_pairs if n_pairs is None else n_pairs
        hom = self.torch.from_numpy(np.ascontiguousarray(hom, np.float64)).to(self.eng.device)
        ssq = self.nan(self.n_pairs)
        status = self.eng.lib.pano_ba_residuals(
            self.eng.ctx(), engine._ptr(self.dev["rows"]), engine._ptr(self.dev["pairs"]),
            n_pairs, engine._ptr(hom), engine._ptr(ssq))
        out = ssq.cpu().numpy()
        _lib.check(status, "pano_ba_residuals")
        return out

    def inputs_unchanged(self):
        return all(np.array_equal(self.dev[k].cpu().numpy().view(np.uint8).ravel(),
                                  np.ascontiguousarray(v).view(np.uint8).ravel())
                   for k, v in self.host.items())


@pytest.fixture(scope="module")
def forged(eng):
    s = _Forged(eng)
    s.jtj, s.jtr, s.work = s.normal()
    s.ssq = s.residuals(s.f["hom_r"])
    f = s.f
    s.m_sums = bm.pair_sums_ordered(f["rows"], f["pairs"], f["jtab"], f["hom_r"])
    s.m_jtj, s.m_jtr = bm.assemble_ordered(s.m_sums, f["pairs"], f["slot"], s.n_active, bm.LAMBDA)
    s.m_ssq = bm.ssq_ordered(f["rows"], f["pairs"], f["hom_r"])
    return s


def _mismatch(got, want):
    bad = np.argwhere(_bits(got) != _bits(want))
    return f"{len(bad)} of {got.size} differ, first at {bad[:5].tolist()}"


def test_residual_sums_have_the_contract_bits(forged):
    s = forged
    assert np.array_equal(_bits(s.ssq), _bits(s.m_ssq)), _mismatch(s.ssq, s.m_ssq)
    # ... and at the Jacobian's own state
    ssq_j = s.residuals(s.f["hom_j"])
    want = bm.ssq_ordered(s.f["rows"], s.f["pairs"], s.f["hom_j"])
    assert np.array_equal(_bits(ssq_j), _bits(want)), _mismatch(ssq_j, want)
    assert not np.array_equal(ssq_j, s.ssq)


def test_pair_sums_have_the_contract_bits(forged):
    s = forged
    assert s.work.shape == (s.n_pairs, 90)
    for p in range(s.n_pairs):
        assert np.array_equal(_bits(s.work[p]), _bits(s.m_sums[p])), \
            (p, s.f["pairs"][p].tolist(), _mismatch(s.work[p], s.m_sums[p]))


def test_assembled_system_has_the_contract_bits(forged):
    s = forged
    assert np.array_equal(_bits(s.jtj), _bits(s.m_jtj)), _mismatch(s.jtj, s.m_jtj)
    assert np.array_equal(_bits(s.jtr), _bits(s.m_jtr)), _mismatch(s.jtr, s.m_jtr)
    # the assembly alone, from the kernel's own pair sums
    jtj, jtr = bm.assemble_ordered(s.work, s.f["pairs"], s.f["slot"], s.n_active, bm.LAMBDA)
    assert np.array_equal(_bits(s.jtj), _bits(jtj)) and np.array_equal(_bits(s.jtr), _bits(jtr))


def test_kernels_match_the_independent_model(forged):
    """Measured on an MI355X: J^T J 1.4e-15, J^T r 1.1e-15, ssq 5.3e-15 (the figures of the
    ordered model on the CPU, whose bits the kernels have), against the bound of 1e-12."""
    s, f = forged, forged.f
    want_jtj, want_jtr = bm.normal_equations(f["cameras"], f["res_cameras"], f["matches"])
    want_ssq = bm.pair_ssq(f["res_cameras"], f["matches"])
    dev, dev_r, dev_s = bm.scaled_deviations(s.jtj, s.jtr, s.ssq, want_jtj, want_jtr, want_ssq)
    print(f"kernels against the independent model: J^T J {dev:.2e}, J^T r {dev_r:.2e}, "
          f"ssq {dev_s:.2e}")
    assert dev <= 1e-12 and dev_r <= 1e-12 and dev_s <= 1e-12


def test_every_entry_is_written_and_nothing_outside_a_region_is_read(forged):
    s, f = forged, forged.f
    assert np.all(np.isfinite(s.jtj)) and np.all(np.isfinite(s.jtr))
    assert np.all(np.isfinite(s.work)) and np.all(np.isfinite(s.ssq))
    assert np.array_equal(_bits(s.jtj), _bits(s.jtj.T))
    slot = f["slot"]
    shared = {(slot[a], slot[b]) for a, b in f["pairs"][:, :2].tolist()}
    lonely = [(r, c) for r in range(s.n_active) for c in range(s.n_active)
              if r != c and (r, c) not in shared and (c, r) not in shared]
    assert len(lonely) == 4
    for r, c in lonely:
        assert np.all(_bits(s.jtj[6 * r:6 * r + 6, 6 * c:6 * c + 6]) == 0)     # +0.0
    empty = np.nonzero(f["pairs"][:, 3] == 0)[0]
    assert len(empty) == 1
    assert np.all(_bits(s.work[empty[0]]) == 0) and _bits(s.ssq[empty])[0] == 0


@pytest.mark.parametrize("n_active", [1, 3])
def test_no_pairs_gives_lambda_on_the_diagonal(forged, n_active):
    for inputs in (True, False):                        # null rows, pairs, tables and work too
        jtj, jtr, work = forged.normal(n_pairs=0, n_active=n_active, inputs=inputs)
        assert work.shape == (0, 90)
        assert np.array_equal(_bits(jtj), _bits(bm.LAMBDA * np.eye(6 * n_active)))
        assert np.all(_bits(jtr) == 0)
    assert np.all(np.isnan(forged.residuals(forged.f["hom_r"], n_pairs=0)))   # nothing to write


def test_runs_repeat_their_bytes_and_leave_the_inputs_alone(forged):
    s = forged
    jtj, jtr, work = s.normal()
    ssq = s.residuals(s.f["hom_r"])
    for got, first in ((jtj, s.jtj), (jtr, s.jtr), (work, s.work), (ssq, s.ssq)):
        assert np.array_equal(_bits(got), _bits(first))
    assert s.inputs_unchanged()


@pytest.mark.parametrize("fault", ["n_active = 0", "n_pairs = -1", "null slot"])
def test_refusals_write_nothing(forged, fault):
    from pano360_amd import _lib
    kw = {"n_active = 0": dict(n_active=0), "n_pairs = -1": dict(n_pairs=-1),
          "null slot": dict(slot=False)}[fault]
    with pytest.raises(_lib.PanoError, match="pano_ba_normal"):
        forged.normal(**kw)
    jtj, jtr, _ = forged.normal(refused=True, **kw)
    assert np.all(np.isnan(jtj)) and np.all(np.isnan(jtr))
    if fault == "n_pairs = -1":
        with pytest.raises(_lib.PanoError, match="pano_ba_residuals"):
            forged.residuals(forged.f["hom_r"], n_pairs=-1)
    assert forged.inputs_unchanged()
    jtj, jtr, work = forged.normal()                    # and the next call is served
    assert np.array_equal(_bits(jtj), _bits(forged.jtj))
