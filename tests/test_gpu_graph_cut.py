"""GPU: the overlap seam (csrc/graphcut.hip through blend.graph_cut, blend.graph_cut_device,
blend.alpha_blend and blend.blend_overlap_device).

Labels are integers and the class sweep is an exact restatement of the reference's heap loop, so
every comparison here is equality: the int8 label grid against what the reference handed to its
resize (tests/golden/graph_cut_*.npz, tools/gen_graph_cut_golden.py), on the resident path and,
forced, on the tiled path; the uint8 mask byte for byte; a full-size case against
tests/graph_cut_model.py, whose heap loop cross-checks its sweep there."""
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import graph_cut_model as gm  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "graph_cut_*.npz")))
RESIDENT, TILED = 1, 2


def load(path):
    g = dict(np.load(path))
    dtype = np.dtype(str(g["dtype"]))
    return g["img1"].astype(dtype), g["img2"].astype(dtype), int(g["shrink"]), g


def on_device(eng, img1, img2, shrink, path=0):
    """graph_cut_device on host arrays: (mask, labels) as host arrays."""
    import torch
    from pano360_amd import blend
    mask, labels = blend.graph_cut_device(torch.from_numpy(img1).to(eng.device),
                                          torch.from_numpy(img2).to(eng.device), shrink, eng,
                                          want_labels=True, path=path)
    return mask.cpu().numpy(), labels.cpu().numpy()


@pytest.fixture(scope="module", params=FIXTURES, ids=lambda p: os.path.basename(p)[10:-4])
def golden(request):
    return load(request.param)


def test_fixtures_present():
    assert len(FIXTURES) == 7, FIXTURES


@pytest.mark.parametrize("path", (RESIDENT, TILED), ids=("resident", "tiled"))
def test_labels_and_mask_equal_the_reference(eng, golden, path):
    """Every cell of the label grid and every byte of the mask, both flood kernels."""
    img1, img2, shrink, g = golden
    if gm.border_of(shrink) == 1:
        path = 0                                   # all preset: nothing floods
    mask, labels = on_device(eng, img1, img2, shrink, path)
    assert labels.dtype == np.int8 and labels.shape == g["labels"].shape
    wrong = int((labels != g["labels"]).sum())
    print(f"shrink {shrink}, grid {labels.shape}: {wrong} cells differ, "
          f"{int((mask != g['mask']).sum())} mask bytes differ")
    assert wrong == 0
    assert mask.dtype == np.uint8 and np.array_equal(mask, g["mask"])


def test_host_call_equals_the_reference(eng, golden):
    from pano360_amd import blend
    img1, img2, shrink, g = golden
    mask = blend.graph_cut(img1, img2, shrink)
    assert mask.dtype == np.uint8 and mask.shape == g["mask"].shape
    assert np.array_equal(mask, g["mask"])


@pytest.mark.parametrize("shrink", (5, 1))
def test_full_size_against_the_model(eng, shrink):
    """The reference main()'s overlap, 1080 x 976 x 3: shrink=5 takes the resident path (a
    216 x 195 grid), shrink=1 the tiled one (1.05 M cells); both are also forced onto the tiled
    path.  The model's heap loop cross-checks its sweep at shrink=5."""
    img1, img2 = gm.smooth_pair(1080, 976, 3, 2024, np.int16, noise=2.0)
    level = gm.levels(img1, img2, shrink)
    border = gm.border_of(shrink)
    want, worked = gm.flood_sweep(level, border, want_stats=True)
    share = [float(np.mean(want == c)) for c in (-1, 1)]
    print(f"shrink {shrink}: grid {want.shape}, shares {share}, classes that worked {worked}")
    assert min(share) >= 0.10 and worked >= 20
    if shrink == 5:
        assert np.array_equal(gm.flood_heap(level, border), want)
    for path in (0, TILED):
        mask, labels = on_device(eng, img1, img2, shrink, path)
        assert np.array_equal(labels, want), (shrink, path, int((labels != want).sum()))
        assert np.array_equal(mask, gm.mask_from_labels(want, 1080, 976))


def test_levels_equal_the_model(eng):
    """pano_seam_levels alone, every dtype, with the alpha rule and a crop."""
    import torch
    from pano360_amd import blend
    for k, dtype in enumerate(gm.DTYPES):
        chans = 3 if dtype == np.uint8 else 4
        pair = gm.smooth_pair(67, 83, 3, 300 + k, dtype, noise=2.0)
        if chans == 4:
            pair = gm.with_alpha_holes(pair, 400 + k)
        for shrink in (1, 3):
            level, bad = blend.seam_levels_device(torch.from_numpy(pair[0]).to(eng.device),
                                                  torch.from_numpy(pair[1]).to(eng.device),
                                                  shrink, eng)
            assert int(bad.item()) == 0
            assert np.array_equal(level.cpu().numpy(), gm.levels(pair[0], pair[1], shrink)), dtype


def test_values_outside_the_domain_are_refused_on_the_device(eng):
    import torch
    from pano360_amd import blend
    a, b = gm.smooth_pair(40, 60, 3, 5, np.float32)
    for value in (0.5, 256.0, -1.0, float("nan")):
        bad = a.copy()
        bad[7, 9, 1] = value
        with pytest.raises(NotImplementedError):
            blend.graph_cut_device(torch.from_numpy(bad).to(eng.device),
                                   torch.from_numpy(b).to(eng.device), 2, eng)


def test_same_input_same_bytes(eng):
    img1, img2 = gm.noise_pair(200, 300, 3, 9)
    for path in (RESIDENT, TILED):
        first = on_device(eng, img1, img2, 1, path)
        again = on_device(eng, img1, img2, 1, path)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


def test_alpha_blend_bytes_are_numpys(eng):
    from pano360_amd import blend
    rng = np.random.default_rng(3)
    img1 = rng.integers(0, 256, (37, 53, 3)).astype(np.uint8)
    img2 = rng.integers(0, 256, (37, 53, 3)).astype(np.uint8)
    ramp = np.linspace(1, 0, 53).reshape((1, 53, 1))
    assert np.array_equal(blend.alpha_blend(img1, img2),
                          (img1 * ramp + img2 * (1 - ramp)).astype("uint8"))
    for dtype in (np.float32, np.float64):
        mask = rng.random((37, 53, 1)).astype(dtype)
        for a, b in ((img1, img2), (img1.astype(np.int16), img2.astype(np.int16)),
                     (img1.astype(np.int32), img2.astype(np.int32)),
                     (img1.astype(np.float32), img2.astype(np.float32))):
            want = (a * mask + b * (1 - mask)).astype("uint8")
            got = blend.alpha_blend(a, b, mask)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (dtype, a.dtype)
            assert np.array_equal(gm.alpha_blend(a, b, mask), want)
    full = rng.random((37, 53, 3))
    assert np.array_equal(blend.alpha_blend(img1, img2, full),
                          (img1 * full + img2 * (1 - full)).astype("uint8"))


@pytest.mark.parametrize("blender", ("poisson", "laplacian"))
def test_blend_overlap_equals_the_public_calls_composed(eng, blender):
    """blend.py:219-226 by hand through the host API against blend_overlap_device."""
    import torch
    from pano360_amd import blend
    delta = 140
    img1, img2 = gm.smooth_pair(128, 200, 3, 77, np.uint8, noise=2.0)
    left, right = img1[:, -delta:], img2[:, :delta]
    mask = blend.graph_cut(left.astype(np.int16), right.astype(np.int16))
    share = float(np.mean(mask > 127))
    print(f"{blender}: img1 owns {share:.3f} of the overlap")
    assert 0.05 < share < 0.95
    if blender == "poisson":
        overlap = blend.poisson_blend(left.copy(), right.copy(), mask[..., 0] > 127)
    else:
        overlap = blend.laplacian_blending(left, right, mask / 255.0)
    want = np.concatenate([img1[:, :-delta], overlap.astype("uint8"), img2[:, delta:]], axis=1)
    got = blend.blend_overlap_device(torch.from_numpy(img1).to(eng.device),
                                     torch.from_numpy(img2).to(eng.device), delta, blender)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
