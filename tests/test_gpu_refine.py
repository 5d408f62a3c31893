"""GPU: pano_ba_refine (csrc/refine.hip) through its native entry on the forged pair tables of
tests/refine_cases.py, ``bundle_adj.refine`` against the NumPy model's loop on the noisy ring,
and ``--register --refine-lens 1`` from images to mosaic against the same steps through the
Python API.  The model is tests/refine_model.py; outputs are prefilled with NaN."""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import refine_cases as rc  # noqa: E402
import refine_model as rm  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = -1


def _call(eng, case, k, delta=rc.DELTA, n_pairs=None, n_cameras=None, null=None, fill=np.nan,
          n_rows=None):
    """pano_ba_refine into a prefilled buffer: (status, out [P][70] on the host)."""
    import torch
    from pano360_amd import engine
    dev = {key: torch.from_numpy(np.ascontiguousarray(case[key])).to(eng.device)
           for key in ("rows", "table", "cams")}
    assert dev["table"].dtype == torch.int32 and dev["rows"].dtype == torch.float64
    out = torch.full((len(case["table"]), rm.TERMS), fill, dtype=torch.float64, device=eng.device)
    ptr = {key: None if key == null else engine._ptr(t) for key, t in dev.items()}
    status = eng.lib.pano_ba_refine(
        eng.ctx(), ptr["rows"], len(case["rows"]) if n_rows is None else n_rows, ptr["table"],
        len(case["table"]) if n_pairs is None else n_pairs, ptr["cams"],
        len(case["cams"]) if n_cameras is None else n_cameras, C.c_double(k[0]), C.c_double(k[1]),
        C.c_double(delta), None if null == "out" else engine._ptr(out))
    return status, out.cpu().numpy()


def test_sums(eng):
    """Every one of the 70 outputs within 1e-12 x the sum of the absolute values of the per-match
    terms summed into it, as the model returns it (reordering at most 4096 f64 additions moves a
    sum by at most n 2^-53 = 4.5e-13 of that), the counts exact, a second call the same bytes.
    Pairs of 0, 1, 63, 64, 65, 256, 257 and 600 matches; in the last one a match at rd = 0 and
    one behind the camera; residuals on both sides of delta."""
    case = rc.forged_sums()
    assert tuple(case["table"][:, 3]) == rc.SUM_COUNTS
    want, mag = rm.pair_sums(case["rows"], case["table"], case["cams"], rc.SUM_K, rc.DELTA)
    counts = case["table"][:, 3]
    assert want[:, 67].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]          # the match behind the camera
    assert np.all((want[2:, 69] > 0) & (want[2:, 69] < counts[2:] - want[2:, 67]))
    status, got = _call(eng, case, rc.SUM_K)
    assert status == 0
    assert np.all(np.isfinite(got))
    assert np.array_equal(got[0], np.zeros(rm.TERMS))                # a pair without matches
    assert np.array_equal(got[:, [67, 69]], want[:, [67, 69]])
    dev = np.abs(got - want) / np.where(mag > 0, mag, 1.0)
    print(f"largest deviation over the terms' absolute sum: {np.max(dev):.2e}")
    assert np.all(np.abs(got - want) <= 1e-12 * mag)
    again = _call(eng, case, rc.SUM_K)[1]
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))


def test_sums_with_a_fold(eng):
    """k1 = -0.4 and an observation at rd = 1.2: h' = 1 - 1.2 rd^2 <= 0 at the first Newton step;
    that match is invalid, the others are summed as the model sums them."""
    case = rc.forged_hp()
    want, mag = rm.pair_sums(case["rows"], case["table"], case["cams"], rc.HP_K, rc.DELTA)
    assert want[0, 67] == 1
    status, got = _call(eng, case, rc.HP_K)
    assert status == 0
    assert np.array_equal(got[:, [67, 69]], want[:, [67, 69]])
    assert np.all(np.abs(got - want) <= 1e-12 * mag)


def test_pair_outside_the_tables_reads_nothing(eng):
    """A pair that names a camera or rows that do not exist: its matches are invalid."""
    case = rc.forged_hp()
    for bad in ((3, 0, 0, 5), (1, -1, 0, 5), (1, 0, 2, 4), (1, 0, -1, 2)):
        forged = dict(case, table=np.array([bad], np.int32))
        status, got = _call(eng, forged, rc.HP_K)
        assert status == 0
        want = np.zeros(rm.TERMS)
        want[67] = bad[3]
        assert np.array_equal(got[0], want), bad


def test_refusals(eng):
    """PANO_EINVAL, and the output as it was."""
    case = rc.forged_hp()
    refused = [dict(null="rows"), dict(null="table"), dict(null="cams"), dict(n_pairs=0),
               dict(n_pairs=-1), dict(n_cameras=0), dict(n_rows=-1), dict(delta=0.0),
               dict(delta=-3.0),
               dict(delta=float("nan")), dict(delta=float("inf"))]
    for kw in refused:
        status, out = _call(eng, case, rc.HP_K, fill=7.25, **kw)
        assert status == EINVAL, kw
        assert np.all(out == 7.25), kw
    assert _call(eng, case, rc.HP_K, null="out")[0] == EINVAL
    assert eng.lib.pano_ba_refine(None, None, 0, None, 1, None, 1, C.c_double(0), C.c_double(0),
                                  C.c_double(3), None) == EINVAL


# 10 x refine_cases.perturbed_movement(): f 2.9e-15 relative, k 8.6e-15, a rotation entry 2.4e-15
TOLERANCE = (2.9e-14, 8.6e-14, 2.4e-14)


def test_refine_against_the_model(eng):
    """The noisy ring, lens_terms = 1: every decision and every lambda the model's, f, k and the
    rotations within 10 x what relative 1e-12 noise on the model's per-pair sums moved the model's
    own result (``refine_cases.perturbed_movement()``: eight seeded reruns on the CPU, every
    decision kept; the largest movements are recorded in DESIGN 5p and repeated in TOLERANCE's
    comment)."""
    from pano360_amd import bundle_adj as ba
    case, want = rc.ring("noisy"), rc.solved("noisy", 1)
    res = ba.refine(case["cameras"], case["matches"], case["index"], lens_terms=1, huber=rc.DELTA)
    assert [h[2] for h in res.history] == [h[2] for h in want["history"]]
    assert [h[1] for h in res.history] == [h[1] for h in want["history"]]
    f = np.array([c.intr[0, 0] for c in res.cameras])
    R = np.stack([c.rot for c in res.cameras])
    dev = (float(np.max(np.abs(f / want["f"] - 1))),
           float(np.max(np.abs(np.array(res.k) - want["k"]))), float(np.max(np.abs(R - want["R"]))))
    print("f %.2e relative, k %.2e, rotations %.2e" % dev)
    assert all(d <= t for d, t in zip(dev, TOLERANCE))
    assert res.n_invalid == want["n_invalid"] and res.inlier_share == want["inlier_share"]
    assert abs(res.rms_after - want["rms_after"]) <= 1e-12
    assert abs(res.rms_before - want["rms_before"]) <= 1e-12
    again = ba.refine(case["cameras"], case["matches"], case["index"], lens_terms=1)
    assert np.array_equal(np.stack([c.rot for c in again.cameras]), R) and again.k == res.k


W, H_ = 160, 90


def test_cli_refine_lens_equals_the_api(tmp_path, monkeypatch):
    """Four rendered 160 x 90 frames: ``--register --refine-lens 1`` gives, byte for byte, the
    ``stitch`` of the registered cameras refined and undistorted through the Python API."""
    import torch
    from PIL import Image as PilImage
    from pano360_amd import bundle_adj as ba
    from pano360_amd import lens, stitcher, synth
    pano = synth.make_frame(7, 1024, 512, "B")
    rots, intrs = synth.make_cameras(4, W, H_, step_deg=20.0, jitter=0.01, seed=3)
    frames = synth.render_rig(pano, rots, intrs, W, H_, torch.device("cuda"))
    src = tmp_path / "rig"
    src.mkdir()
    for k, f in enumerate(frames):
        PilImage.fromarray(f.cpu().numpy()[..., ::-1]).save(src / f"f{k}.png")
    del frames
    monkeypatch.chdir(tmp_path)
    got = stitcher.main([str(src), "-s", "1", "--register", "--refine-lens", "1"])

    with open(tmp_path / "ba_rig_s1.0.pkl", "rb") as fid:
        regions = pickle.load(fid)
    arr = np.load(tmp_path / "matches_rig_s1.0.npz", allow_pickle=True)
    assert len(regions) == len(arr["kpts"]) == 4
    res = ba.refine(regions, stitcher.idx_to_keypoints(arr["matches"], arr["kpts"]), lens_terms=1)
    assert len(res.history) >= 1 and np.isfinite(res.k[0]) and res.k[1] == 0.0
    fixed, focals = lens.undistort_device([r.img for r in res.cameras],
                                          res.lens_models([(W, H_)] * 4), "cubic")
    for reg, frame, focal in zip(res.cameras, fixed, focals):
        reg.img, reg.intr = frame, ba.intrinsics(focal)
    want = stitcher.stitch(res.cameras, stitcher.BLENDERS["multiband"])
    assert got.shape == want.shape and got.size > 0
    assert np.array_equal(got, want)
    # the caches are the registration's, untouched by the refinement
    with open(tmp_path / "ba_rig_s1.0.pkl", "rb") as fid:
        for reg, kept in zip(pickle.load(fid), regions):
            assert np.array_equal(reg.intr, kept.intr) and np.array_equal(reg.rot, kept.rot)
