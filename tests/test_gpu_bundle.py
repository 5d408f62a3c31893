"""GPU: bundle adjustment (csrc/bundle.hip through bundle_adj.traverse).

The kernels against the reference's J^T J, J^T r (at an accepted and at a rejected camera state)
and residuals; ``traverse`` in every mode against the reference's runs (tests/golden/ba_*.npz)
and, at 32 cameras, against the NumPy model that the CPU tests pin to those runs; determinism;
a known answer from frames rendered from true cameras; the CLI from images to mosaic.
Tolerances are ba_model.check_run's (tests/test_bundle_host.py says why).  The frames here are
640 x 360 and are detected on an engine of this module's own or in a child process."""
import glob
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ba_model as bm  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "ba_*.npz")))
MODES = ("none", "incr", "last")
W, H_ = 640, 360


@pytest.fixture(scope="module", params=FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def golden(request):
    return dict(np.load(request.param))


def _system_on_device(golden, res_tag):
    """The kernels on the fixture's final state of its last incr optimize call: J at the
    accepted cameras, r at the `res_tag` cameras."""
    from pano360_amd import bundle_adj as ba
    n = int(golden["n_cameras"])
    acc = bm.cameras_from(golden["sys_acc_index"], golden["sys_acc_intr"], golden["sys_acc_rot"], n)
    res = bm.cameras_from(golden[f"sys_{res_tag}_index"], golden[f"sys_{res_tag}_intr"],
                          golden[f"sys_{res_tag}_rot"], n)
    matches = bm.unflatten_matches(golden)
    iba = ba.IncrementalBundleAdjuster(n, mode="none")
    iba.cameras = acc
    iba.matches = [(int(a), int(b), matches[b][a][0]) for a, b in golden["incr_pairs"]]
    dev = iba._device()
    a = np.array([m[0] for m in iba.matches])
    b = np.array([m[1] for m in iba.matches])
    counts = np.array([len(m[2]) for m in iba.matches])
    pairs = iba._pair_table(a, b, np.array(iba._first), counts)
    idx = [i for i, c in enumerate(acc) if c is not None]
    slot = np.full(n, -1)
    slot[idx] = np.arange(len(idx))
    s_acc, s_res = ba._State.of(acc), ba._State.of(res)
    jtab = ba._jacobian_tables(s_acc.K, s_acc.R, s_acc.Kinv, ba._dr_dvis(s_acc.R), a, b)
    hom_r = ba._pair_homs(s_res.K, s_res.R, s_res.Kinv, a, b)
    work = dev.torch.empty(int(dev.eng.lib.pano_ba_work_bytes(len(a))), dtype=dev.torch.uint8,
                           device=dev.dev)
    jtj, jtr = dev.download(*dev.normal(pairs, len(a), dev.upload(slot, np.int32), len(idx),
                                        jtab, hom_r, work))
    ssq = dev.download(dev.pair_ssq(pairs, len(a), hom_r))[0]
    return jtj, jtr, ssq, counts


@pytest.mark.parametrize("tag", ["acc", "rej"])
def test_kernels_match_reference(golden, tag):
    from pano360_amd import bundle_adj as ba
    jtj, jtr, ssq, counts = _system_on_device(golden, tag)
    want = golden["sys_jtj"] + ba.LM_LAMBDA * np.eye(len(golden["sys_jtj"]))
    res = golden[f"sys_res_{tag}"]
    d = np.sqrt(np.diag(want))
    dev = np.max(np.abs(jtj - want) / np.outer(d, d))
    dev_r = np.max(np.abs(jtr - golden[f"sys_jtr_{tag}"]) / (d * np.sqrt(np.sum(res ** 2))))
    ends = np.cumsum(counts)
    want_ssq = np.array([np.sum(res[2 * (e - c):2 * e] ** 2) for e, c in zip(ends, counts)])
    dev_s = np.max(np.abs(ssq / want_ssq - 1))
    print(f"largest deviation: J^T J {dev:.2e}, J^T r {dev_r:.2e}, ssq {dev_s:.2e}")
    assert dev <= 1e-12 and dev_r <= 1e-12 and dev_s <= 1e-12
    assert np.array_equal(jtj, jtj.T)


def _traverse(matches, n, mode, imgs=None):
    """bundle_adj.traverse with its adjuster kept: (index, cameras, adjuster)."""
    from pano360_amd import bundle_adj as ba
    made = []

    class Kept(ba.IncrementalBundleAdjuster):
        def __init__(self, *args, **kw):
            super().__init__(*args, **kw)
            made.append(self)
    orig = ba.IncrementalBundleAdjuster
    ba.IncrementalBundleAdjuster = Kept
    try:
        imgs = imgs if imgs is not None else [np.full(1, i) for i in range(n)]
        cams = ba.traverse(imgs, matches, badjust=mode)
    finally:
        ba.IncrementalBundleAdjuster = orig
    return [int(c.img[0]) for c in cams], cams, made[0]


@pytest.mark.parametrize("mode", MODES)
def test_traverse_matches_reference(golden, mode):
    index, cams, iba = _traverse(bm.unflatten_matches(golden), int(golden["n_cameras"]), mode)
    bm.check_run(golden, mode, index, cams, iba.history, [(a, b) for a, b, _ in iba.matches])


def test_traverse_at_scale_matches_model():
    matches, _ = bm.synthetic_matches(77, 32, 2000, reach=2)
    assert sum(len(v) for v in matches.values()) // 2 == 64
    index, cams, iba = _traverse(matches, 32, "incr")
    want = bm.run_record(*bm.traverse(32, matches, "incr"))
    bm.check_run(want, "incr", index, cams, iba.history, [(a, b) for a, b, _ in iba.matches],
                 prefix="m", **bm.SCALE_TOLS)


def test_traverse_is_deterministic():
    golden = dict(np.load(FIXTURES[0]))
    runs = [_traverse(bm.unflatten_matches(golden), int(golden["n_cameras"]), "incr")[1]
            for _ in range(2)]
    for c0, c1 in zip(*runs):
        assert np.array_equal(c0.rot, c1.rot) and np.array_equal(c0.intr, c1.intr)
    first = _system_on_device(golden, "rej")
    again = _system_on_device(golden, "rej")
    for x, y in zip(first, again):
        assert np.array_equal(x, y)


def _rig(n=6, step=30.0):
    from pano360_amd import synth
    pano = synth.make_frame(7, 4096, 2048, "B")
    rots, intrs = synth.make_cameras(n, W, H_, step_deg=step, jitter=0.01, seed=3)
    return pano, rots, intrs


def _angle(rot):
    return np.degrees(np.arccos(np.clip((np.trace(rot) - 1) / 2, -1, 1)))


def test_known_answer_from_rendered_frames():
    """Six frames 30 degrees apart.  Observed: relative rotations within 0.28 degrees (between
    the farthest cameras: a 0.23 % focal error scales the 150 degree sweep by about that much),
    focal within 0.23 %.  Bounds: 0.5 degrees, 1 %."""
    from pano360_amd import bundle_adj as ba
    from pano360_amd import engine, features, stitcher, synth
    pano, rots, intrs = _rig()
    eng = engine.Engine()
    frames = synth.render_rig(pano, rots, intrs, W, H_, eng.device)
    kpts, matches = features.matching(frames, detect=features.sift_detector(eng))
    cams = ba.traverse(frames, stitcher.idx_to_keypoints(matches, kpts), badjust="incr")
    assert len(cams) == len(frames)
    order = [next(k for k, f in enumerate(frames) if f is c.img) for c in cams]
    worst = 0.0
    for p in range(len(cams)):
        for q in range(p + 1, len(cams)):
            i, j = order[p], order[q]
            got = cams[p].rot @ cams[q].rot.T
            true = rots[i] @ rots[j].T
            worst = max(worst, _angle(got @ true.T))
    focal = intrs[0][0, 0]
    f_err = max(abs(c.intr[0, 0] / focal - 1) for c in cams)
    print(f"relative rotations within {worst:.4f} deg, focal within {100 * f_err:.3f} %")
    assert worst <= 0.5
    assert f_err <= 0.01


def test_cli_registers_and_reuses_caches(tmp_path):
    from PIL import Image as PilImage
    from pano360_amd import synth
    import torch
    pano, rots, intrs = _rig(4, 30.0)
    frames = synth.render_rig(pano, rots, intrs, W, H_, torch.device("cuda"))
    src = tmp_path / "rig"
    src.mkdir()
    for k, f in enumerate(frames):
        PilImage.fromarray(f.cpu().numpy()[..., ::-1]).save(src / f"f{k}.png")
    del frames
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import stitcher; "
            "m = stitcher.main([%r, '-s', '1', '-b', 'linear', '--register']); np.save(sys.argv[1], m)"
            % (ROOT, str(src)))
    outs = []
    for run in range(2):
        out = tmp_path / f"mosaic{run}.npy"
        subprocess.run([sys.executable, "-c", code, str(out)], cwd=tmp_path, check=True,
                       timeout=300)
        outs.append(np.load(out))
        if run == 0:
            assert (tmp_path / "matches_rig_s1.0.npz").exists()
            pkl = tmp_path / "ba_rig_s1.0.pkl"
            assert pkl.exists()
            stamp = pkl.stat().st_mtime_ns
            sys.path.insert(0, ROOT)
            import bundle_adj
            with open(pkl, "rb") as fid:
                regions = pickle.load(fid)
            assert len(regions) == 4
            for reg in regions:
                assert isinstance(reg, bundle_adj.Image)
                assert isinstance(reg.img, np.ndarray) and reg.img.dtype == np.uint8
                assert reg.img.shape == (H_, W, 3)
    assert pkl.stat().st_mtime_ns == stamp, "the camera cache was written again"
    assert outs[0].size > 0 and outs[0].ndim == 3
    assert np.array_equal(outs[0], outs[1])
