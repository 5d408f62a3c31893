"""CPU: bundle adjustment's host helpers and the NumPy model of its kernel contract and LM loop
(tests/ba_model.py) against the reference's outputs in tests/golden/ba_*.npz
(tools/gen_ba_golden.py), ``stitcher.idx_to_keypoints`` and the new symbols' signatures; the
model's second restatement, in the contract's order of additions (what
tests/test_gpu_bundle_forged.py compares the kernels with bit for bit), against the first on a
forged pair table.

Tolerances.  Entries of J^T J and J^T r are compared relative to their Cauchy-Schwarz scale
(sqrt(A_ii A_jj) and sqrt(A_ii r.r)): the entries range over six decades (focal columns against
rotation columns), so one scale for the whole matrix would test nothing for the small ones.
A traverse (ba_model.check_run): accept decisions, iteration counts, kept pairs and cameras
reached exactly; losses to 1e-9 relative, focal to 1e-9 relative, rotation entries to 1e-8.
The model and the reference differ only in summation order and in the last ulp of NumPy's small
products.  Over a whole traverse that drift grew to 7e-11 in a loss and 2.8e-9 in a rotation
entry: the latter on ring8, where the gate splits the cameras into three groups with no pair
between them, so LM's damping alone fixes their relative rotation.  Everywhere else rotations
agreed to 1e-12 and focals to 2e-13."""
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ba_model as bm  # noqa: E402
from pano360_amd import bundle_adj as ba  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "ba_*.npz")))
MODES = ("none", "incr", "last")


@pytest.fixture(scope="module", params=FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def golden(request):
    return dict(np.load(request.param))


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def _scaled_dev(jtj, jtr, want_jtj, want_jtr, rr):
    d = np.sqrt(np.abs(np.diag(want_jtj)))
    dev = np.max(np.abs(jtj - want_jtj) / np.outer(d, d))
    dev_r = np.max(np.abs(jtr - want_jtr) / (d * np.sqrt(rr)))
    return float(dev), float(dev_r)


def test_fixtures_present():
    assert len(FIXTURES) >= 2


def test_focal_matches_reference(golden):
    got = np.array([ba.get_focal(h) for h in golden["focal_hom"]])
    assert _rel(got, golden["focal_ref"]) <= 1e-12


def test_angles_and_derivatives_match_reference(golden):
    for rot, want, dr in zip(golden["angle_rot"], golden["angle_ref"], golden["drdv_ref"]):
        got = ba.mat_to_angle(rot)
        assert np.max(np.abs(got - want)) <= 1e-12 * max(np.max(np.abs(want)), 1e-300)
        assert np.max(np.abs(ba.dr_dvi(rot) - dr)) <= 1e-12 * np.max(np.abs(dr))


def test_straighten_matches_reference(golden):
    for rots, want in zip(golden["straighten_in"], golden["straighten_ref"]):
        got = np.stack(ba.straighten(list(rots)))
        assert np.max(np.abs(got - want)) <= 1e-12


def test_params_round_trip():
    rng = np.random.default_rng(3)
    for _ in range(5):
        prm = np.r_[rng.uniform(300, 2000), rng.normal(0, 5, 2), rng.normal(0, 0.8, 3)]
        back = ba.camera_to_params(ba.params_to_camera(prm))
        assert np.allclose(back, prm, rtol=1e-12, atol=1e-12)


def _system_state(golden):
    n = int(golden["n_cameras"])
    acc = bm.cameras_from(golden["sys_acc_index"], golden["sys_acc_intr"], golden["sys_acc_rot"], n)
    rej = bm.cameras_from(golden["sys_rej_index"], golden["sys_rej_intr"], golden["sys_rej_rot"], n)
    matches = bm.unflatten_matches(golden)
    pairs = [(int(a), int(b), matches[b][a][0]) for a, b in golden["incr_pairs"]]
    return acc, rej, pairs


def test_model_normal_equations_match_reference(golden):
    acc, rej, pairs = _system_state(golden)
    want = golden["sys_jtj"] + ba.LM_LAMBDA * np.eye(len(golden["sys_jtj"]))
    for cams, tag in ((acc, "acc"), (rej, "rej")):
        jtj, jtr = bm.normal_equations(acc, cams, pairs)
        rr = float(np.sum(golden[f"sys_res_{tag}"] ** 2))
        dev, dev_r = _scaled_dev(jtj, jtr, want, golden[f"sys_jtr_{tag}"], rr)
        assert dev <= 1e-12 and dev_r <= 1e-12, (tag, dev, dev_r)


def test_model_residuals_match_reference(golden):
    acc, rej, pairs = _system_state(golden)
    sizes = np.cumsum([0] + [len(m) for _, _, m in pairs])
    for cams, tag in ((acc, "acc"), (rej, "rej")):
        res = golden[f"sys_res_{tag}"]
        want = np.array([np.sum(res[2 * s:2 * e] ** 2) for s, e in zip(sizes[:-1], sizes[1:])])
        assert _rel(bm.pair_ssq(cams, pairs), want) <= 1e-12


@pytest.mark.parametrize("mode", MODES)
def test_model_traverse_matches_reference(golden, mode):
    matches = bm.unflatten_matches(golden)
    index, cams, adj = bm.traverse(int(golden["n_cameras"]), matches, mode)
    bm.check_run(golden, mode, index, cams, adj.history, [(a, b) for a, b, _ in adj.matches])


def test_fixtures_exercise_gate_and_unreached_camera(golden):
    keys = {tuple(sorted(k)) for k in golden["in_keys"].tolist()}
    kept = {tuple(sorted(p)) for p in golden["incr_pairs"].tolist()}
    assert keys - kept, "no pair was left out by the gate"
    assert not all(golden["incr_opt_accepted"]), "no step was rejected"


def test_a_fixture_has_an_unreached_camera():
    assert any(len(np.load(p)["incr_index"]) < int(np.load(p)["n_cameras"]) for p in FIXTURES)


def test_idx_to_keypoints_round_trips_a_match_file(tmp_path):
    from pano360_amd import features, stitcher
    rng = np.random.default_rng(9)
    kpts = [rng.normal(0, 100, (n, 2)).astype(np.float32) for n in (40, 30, 50)]
    found = {}
    for (i, j) in ((0, 1), (1, 2)):
        m = np.stack([rng.choice(len(kpts[i]), 12, replace=False),
                      rng.choice(len(kpts[j]), 12, replace=False)], axis=1).astype(np.int32)
        found[(i, j)] = (m, np.eye(3) + rng.normal(0, 0.01, (3, 3)))
    kpt_arr, match_arr = features._assemble(kpts, found)
    path = tmp_path / "matches_x.npz"
    np.savez(path, kpts=kpt_arr, matches=match_arr)
    arr = np.load(path, allow_pickle=True)
    got = stitcher.idx_to_keypoints(arr["matches"], arr["kpts"])
    assert list(got) == [0, 1, 2] and list(got[1]) == [0, 2]
    for (i, j), (m, h) in found.items():
        for (p, q, mm, hh) in ((i, j, m, h), (j, i, np.fliplr(m), np.linalg.inv(h))):
            rows, hom, score = got[p][q]
            assert rows.shape == (len(mm), 6) and score == len(mm)
            assert np.array_equal(rows[:, :2], kpts[p][mm[:, 0]])
            assert np.array_equal(rows[:, 3:5], kpts[q][mm[:, 1]])
            assert np.all(rows[:, [2, 5]] == 1.0)
            assert np.array_equal(hom, hh)


# ------------------------------------------------------------------ the ordered model
@pytest.fixture(scope="module")
def forged():
    return bm.forged_system()


def test_wave_sum_model_is_the_xor_butterfly():
    x = 2.0 ** -np.arange(64.0)                     # the sum, 2 - 2^-63, is not a float64
    want = x.copy()
    for off in (32, 16, 8, 4, 2, 1):
        want = np.array([want[k] + want[k ^ off] for k in range(64)])
    got = bm.wave_sum_model(x)
    assert np.array_equal(got, want) and np.all(got == got[0])
    # 1 + 2^-53 + 2^-53: the butterfly pairs lane 0 with 32, so the two halves of an ulp meet
    # the 1.0 one at a time and are lost; added to each other first they would survive
    y = np.zeros(64)
    y[0], y[32], y[16] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert bm.wave_sum_model(y)[0] == 1.0
    y[32], y[48] = 0.0, 2.0 ** -53                  # lanes 16 and 48 meet first: an ulp survives
    assert bm.wave_sum_model(y)[0] == 1.0 + 2.0 ** -52
    assert bm.wave_sum_model(np.ones((3, 2, 64))).shape == (3, 2, 64)


def test_forged_system_has_the_cases_the_recorded_runs_lack(forged):
    pairs, slot = forged["pairs"], forged["slot"]
    assert sorted(pairs[:, 3].tolist()) == sorted([0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 513,
                                                   1000, 90, 120])
    assert (slot == -1).sum() == 3 and forged["n_active"] == 6
    assert all(slot[c] != c for c in range(len(slot)))
    assert np.all(slot[pairs[:, :2]] >= 0)
    hub = np.sum(pairs[:, :2] == 5, axis=0)
    assert hub.sum() == 6 and hub.min() >= 1                    # as a and as b
    assert np.any(pairs[:, 0] < pairs[:, 1]) and np.any(pairs[:, 0] > pairs[:, 1])
    keys = [tuple(p) for p in pairs[:, :2].tolist()]
    assert any((b, a) in keys for a, b in keys)                 # one pair in both orders
    assert np.any(np.diff(pairs[:, 2]) < 0)                     # `first` is not monotonic
    rows = forged["rows"]
    inside = np.zeros(len(rows), bool)
    for _, _, first, count in pairs.tolist():
        assert not inside[first:first + count].any()            # regions do not overlap
        inside[first:first + count] = True
    assert np.all(np.isfinite(rows[inside])) and np.all(np.isnan(rows[~inside]))
    assert not inside[0] and not inside[-1]
    edges = np.nonzero(np.diff(inside.astype(int)) == 1)[0]     # a gap before every region
    assert len(edges) == np.sum(pairs[:, 3] > 0)
    assert not np.array_equal(forged["hom_j"], forged["hom_r"])
    assert np.array_equal(forged["jtab"][:, :9], forged["hom_j"])


def test_ordered_model_agrees_with_the_independent_model(forged):
    """The two restatements share no summation: ba_model.normal_equations and pair_ssq use matrix
    products and np.sum, the ordered model the contract's lanes, butterflies and pair order.  In
    the scaled measures of test_kernels_match_reference they agree on the forged input to
    J^T J 1.4e-15, J^T r 1.1e-15, ssq 5.3e-15 (measured), against that test's 1e-12."""
    f = forged
    sums = bm.pair_sums_ordered(f["rows"], f["pairs"], f["jtab"], f["hom_r"])
    jtj, jtr = bm.assemble_ordered(sums, f["pairs"], f["slot"], f["n_active"], bm.LAMBDA)
    ssq = bm.ssq_ordered(f["rows"], f["pairs"], f["hom_r"])
    want_jtj, want_jtr = bm.normal_equations(f["cameras"], f["res_cameras"], f["matches"])
    want_ssq = bm.pair_ssq(f["res_cameras"], f["matches"])
    assert np.all(np.isfinite(sums)) and np.all(np.isfinite(ssq))        # no NaN row was read
    dev, dev_r, dev_s = bm.scaled_deviations(jtj, jtr, ssq, want_jtj, want_jtr, want_ssq)
    print(f"ordered model against the independent one: J^T J {dev:.2e}, J^T r {dev_r:.2e}, "
          f"ssq {dev_s:.2e}")
    assert dev <= 1e-12 and dev_r <= 1e-12 and dev_s <= 1e-12
    assert np.array_equal(jtj, jtj.T)
    # the residual sums of the Jacobian's own state, through the other entry of the model
    ssq_j = bm.ssq_ordered(f["rows"], f["pairs"], f["hom_j"])
    want_j = bm.pair_ssq(f["cameras"], f["matches"])
    some = want_j != 0
    assert np.max(np.abs(ssq_j[some] / want_j[some] - 1)) <= 1e-12 and np.all(ssq_j[~some] == 0)


def test_the_order_of_the_additions_shows_in_the_bits(forged):
    """What a comparison bit for bit can see that 1e-12 cannot: the same terms of the residual
    sums added one after the other, pairwise by np.sum, or with the butterfly's offsets taken
    in ascending order, end in other bits than the contract's order on several of the pairs."""
    f = forged
    want = bm.ssq_ordered(f["rows"], f["pairs"], f["hom_r"])
    serial, pairwise, upward = np.zeros(len(want)), np.zeros(len(want)), np.zeros(len(want))
    lane = np.arange(64)
    for p, (_, _, first, count) in enumerate(f["pairs"].tolist()):
        m = f["rows"][first:first + count]
        t = bm._mul_p(f["hom_r"][p], m[:, 2], m[:, 3])
        rx, ry = m[:, 0] - t[0] / t[2], m[:, 1] - t[1] / t[2]
        val = rx * rx + ry * ry
        for v in val:
            serial[p] = serial[p] + v
        pairwise[p] = np.sum(val)
        acc = bm._padded(val, count).reshape(-1, 4, 64).sum(axis=0)
        for off in (1, 2, 4, 8, 16, 32):
            acc = acc + acc[:, lane ^ off]
        upward[p] = ((acc[0, 0] + acc[1, 0]) + acc[2, 0]) + acc[3, 0]
    for other in (serial, pairwise, upward):
        assert np.max(np.abs(other[1:] / want[1:] - 1)) <= 1e-12
        assert np.sum(other != want) >= 3


def test_ordered_model_structure(forged):
    f = forged
    pairs, slot = f["pairs"], f["slot"]
    sums = bm.pair_sums_ordered(f["rows"], pairs, f["jtab"], f["hom_r"])
    empty = int(np.nonzero(pairs[:, 3] == 0)[0][0])
    assert not sums[empty].any()
    jtj, jtr = bm.assemble_ordered(sums, pairs, slot, f["n_active"], 5.0)
    shared = {(slot[a], slot[b]) for a, b in pairs[:, :2].tolist()}
    lonely = [(r, c) for r in range(6) for c in range(6)
              if r != c and (r, c) not in shared and (c, r) not in shared]
    assert len(lonely) == 4                                     # (2, 6), (3, 8) and transposes
    for r, c in lonely:
        assert not jtj[6 * r:6 * r + 6, 6 * c:6 * c + 6].any()
    # no pairs: lambda I and a zero right-hand side
    none = np.zeros((0, 4), np.int32)
    for n_active in (1, 3):
        jtj0, jtr0 = bm.assemble_ordered(np.zeros((0, 90)), none, slot, n_active, 5.0)
        assert np.array_equal(jtj0, 5.0 * np.eye(6 * n_active)) and not jtr0.any()
    # a pair of fewer rows than a chunk is the plain butterfly of its products
    one = int(np.nonzero(pairs[:, 3] == 1)[0][0])
    jx, jy, rx, ry = bm._columns(f["rows"][pairs[one, 2]:pairs[one, 2] + 1], f["jtab"][one],
                                 f["hom_r"][one])
    assert sums[one][0] == (jx[0] * jx[0] + jy[0] * jy[0])[0]
    assert sums[one][89] == (jx[11] * rx + jy[11] * ry)[0]


def test_traverse_without_pairs_raises():
    with pytest.raises(ValueError):
        ba.traverse([None, None], {})
