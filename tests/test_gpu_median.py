"""GPU: the median blend (fused from the frames, and on patches of the blender protocol) against
``median_model``'s restatement of its contract, bit for bit: mosaics and valid masks."""
import numpy as np
import pytest

import median_model
from conftest import SCENES, load_golden, scene_inputs
from median_cases import bl_patches, ghost_rig

pytestmark = pytest.mark.gpu

OWN_LIST = 256          # csrc/blend.hip: the cameras a block's list holds


def fused(eng, imgs, rots, intrs, mr, tol, **kw):
    from pano360_amd import engine
    plan = engine.Plan([im.shape[:2] for im in imgs], rots, intrs, False, mr)
    mosaic, _, valid, _ = eng.stitch(eng.upload_frames(imgs), plan, "median", tol=tol, **kw)
    return mosaic.cpu().numpy(), None if valid is None else valid.cpu().numpy().astype(bool)


@pytest.fixture(scope="module")
def scene_patches(oracle):
    """Oracle patches of the golden scenes, warped once."""
    out = {}
    for name in SCENES:
        g = load_golden(name)
        imgs, rots, intrs, mr = scene_inputs(g)
        plan, patches, _ = oracle.warp_all(imgs, rots, intrs, False, mr)
        out[name] = (plan.shape, patches)
    return out


@pytest.mark.parametrize("name", SCENES)
def test_fused_against_the_model(eng, scene_patches, name):
    g = load_golden(name)
    imgs, rots, intrs, mr = scene_inputs(g)
    shape, patches = scene_patches[name]
    for tol in (0, 0.02, 0.1):
        mosaic, valid = fused(eng, imgs, rots, intrs, mr, tol)
        want, _ = median_model.median_blend(patches, shape, tol)
        assert np.array_equal(mosaic, want), tol
        assert np.array_equal(valid, g["lin_valid"]), tol
    mosaic, valid = fused(eng, imgs, rots, intrs, mr, 2)
    assert np.array_equal(mosaic, g["linear_mosaic"]) and np.array_equal(valid, g["lin_valid"])
    # the whole-patch path of the same stitch
    staged, _ = fused(eng, imgs, rots, intrs, mr, 0.1, fused=False)
    assert np.array_equal(staged, median_model.median_blend(patches, shape, 0.1)[0])


def test_stage_api_against_the_model(eng):
    from pano360_amd import stitcher
    g = load_golden("pure")
    shape = tuple(int(v) for v in g["bl_shape"])
    for tol in (0, 0.05, 0.1):
        want, _ = median_model.median_blend(bl_patches(g), shape, tol)
        assert np.array_equal(stitcher.median_blend(bl_patches(g), shape, tol), want), tol
    assert np.array_equal(stitcher.median_blend(bl_patches(g), shape, 2), g["bl_linear"])
    with pytest.raises(ValueError):
        stitcher.median_blend(bl_patches(g), shape, -0.5)


def test_ghost_rig(eng, oracle):
    shape, clean, painted, (rots, intrs, frames, ghosted) = ghost_rig(oracle, 8)
    for imgs, patches in ((frames, clean), (ghosted, painted)):
        want, want_valid = median_model.median_blend(patches, shape, 0.1)
        for path in (True, False):
            mosaic, valid = fused(eng, imgs, rots, intrs, 1400, 0.1, fused=path)
            assert mosaic.shape[:2] == shape and np.array_equal(mosaic, want), path
            assert valid is None or np.array_equal(valid, want_valid)


def block_hits(rects, shape, strip=None):
    """Patch rectangles that meet each 64 x 4 block of the fused kernel's grid over the columns
    ``strip``: the length of the block's camera list."""
    H, W = shape
    c0, c1 = strip if strip is not None else (0, W)
    r = np.asarray(rects)
    return np.array([int(((r[:, 2] < min(bx + 64, c1)) & (r[:, 3] > bx)
                          & (r[:, 0] < min(by + 4, H)) & (r[:, 1] > by)).sum())
                     for by in range(0, H, 4) for bx in range(c0, c1, 64)])


def test_more_samples_than_kept(eng, oracle):
    """260 frames 1.3 degrees apart: a closed mosaic, up to 45 samples a pixel (the kernel keeps
    PANO_MEDIAN_KEEP on chip and consumes the rest in passes) and camera lists of 138 to 166, which
    the kernel prunes by the alpha bound."""
    from pano360_amd import _lib, engine, synth
    imgs, rots, intrs = synth.make_scene(260, 32, 24, step_deg=1.3, seed=11, kind="A")
    oplan, patches, _ = oracle.warp_all(imgs, rots, intrs, False, 1400)
    assert oplan.shape == (27, 192)
    counts = median_model.sample_counts(patches, oplan.shape)
    assert counts.max() > _lib.MEDIAN_KEEP and (counts > _lib.MEDIAN_KEEP).mean() > 0.5
    plan = eng.upload_plan(engine.Plan([im.shape[:2] for im in imgs], rots, intrs, False, 1400))
    hits = block_hits(plan.rects, plan.shape)
    assert 16 < hits.min() and hits.max() <= OWN_LIST        # every block: the pruned list
    frames = eng.upload_frames(imgs)
    for tol in (0.1, 0.5, 2):
        want, want_valid = median_model.median_blend(patches, oplan.shape, tol)
        mosaic, valid = eng.median_fused(frames, plan, tol)
        assert np.array_equal(mosaic.cpu().numpy(), want), tol
        assert np.array_equal(valid.cpu().numpy().astype(bool), want_valid), tol
        if tol == 0.1:
            left, lv = eng.median_fused(frames, plan, tol, strip=(0, 100))
            right, rv = eng.median_fused(frames, plan, tol, strip=(100, 192))
            assert np.array_equal(left[:, :100].cpu().numpy(), want[:, :100])
            assert np.array_equal(right[:, 100:].cpu().numpy(), want[:, 100:])
            assert np.array_equal(lv[:, :100].cpu().numpy().astype(bool), want_valid[:, :100])
            assert np.array_equal(rv[:, 100:].cpu().numpy().astype(bool), want_valid[:, 100:])
    linear = oracle.linear_blend(patches, oplan.shape)
    assert np.array_equal(want, linear)                      # (tol = 2, the last one)


def test_camera_list_longer_than_a_block_holds(eng, oracle):
    """290 frames 0.2 degrees apart: every patch rectangle meets every block, more than the 256 a
    block's camera list holds, so the kernel walks all n cameras, unpruned; up to 290 samples a
    pixel, fourteen overflow passes."""
    from pano360_amd import _lib, engine, synth
    imgs, rots, intrs = synth.make_scene(290, 32, 24, step_deg=0.2, seed=5, kind="A")
    oplan, patches, _ = oracle.warp_all(imgs, rots, intrs, False, 1400)
    plan = eng.upload_plan(engine.Plan([im.shape[:2] for im in imgs], rots, intrs, False, 1400))
    assert plan.shape == oplan.shape
    assert block_hits(plan.rects, plan.shape).min() > OWN_LIST
    W = plan.shape[1]
    assert block_hits(plan.rects, plan.shape, (0, W // 2)).min() > OWN_LIST
    assert block_hits(plan.rects, plan.shape, (W // 2, W)).min() > OWN_LIST
    assert median_model.sample_counts(patches, oplan.shape).max() > 4 * _lib.MEDIAN_KEEP
    frames = eng.upload_frames(imgs)
    for tol in (0.1, 0.5, 2):
        want, want_valid = median_model.median_blend(patches, oplan.shape, tol)
        mosaic, valid = eng.median_fused(frames, plan, tol)
        assert np.array_equal(mosaic.cpu().numpy(), want), tol
        assert np.array_equal(valid.cpu().numpy().astype(bool), want_valid), tol
    assert np.array_equal(want, oracle.linear_blend(patches, oplan.shape))
    want, _ = median_model.median_blend(patches, oplan.shape, 0.1)
    left, _ = eng.median_fused(frames, plan, 0.1, strip=(0, W // 2))
    right, _ = eng.median_fused(frames, plan, 0.1, strip=(W // 2, W))
    assert np.array_equal(left[:, :W // 2].cpu().numpy(), want[:, :W // 2])
    assert np.array_equal(right[:, W // 2:].cpu().numpy(), want[:, W // 2:])


def test_per_camera_colour_tables(eng):
    """--equalize: every camera's own table.  The warp with tables is pinned by its own tests;
    the fused blend must take the samples that warp produces."""
    from pano360_amd import engine, stitcher
    g = load_golden("scene_small_smooth")
    imgs, rots, intrs, mr = scene_inputs(g)
    frames = eng.upload_frames(imgs)
    luts = eng.equalize_gains(frames, rots, intrs)[3]
    plan = eng.upload_plan(engine.Plan([im.shape[:2] for im in imgs], rots, intrs, False, mr))
    patches = stitcher._download_patches(eng.warp_all(frames, plan, luts=luts)[0])
    plain = stitcher._download_patches(eng.warp_all(frames, plan)[0])
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(patches, plain))
    for tol in (0.02, 0.1):
        want, want_valid = median_model.median_blend(patches, plan.shape, tol)
        mosaic, valid = eng.median_fused(frames, plan, tol, luts=luts)
        assert np.array_equal(mosaic.cpu().numpy(), want), tol
        assert np.array_equal(valid.cpu().numpy().astype(bool), want_valid)


@pytest.mark.parametrize("n,step_deg,seed", [(260, 1.3, 11), (290, 0.2, 5)])
def test_per_camera_tables_on_long_camera_lists(eng, oracle, n, step_deg, seed):
    """The two rigs above - camera lists the kernels prune by the alpha bound, and lists longer
    than a block holds - with a colour table per camera, rows all different: the three fused
    blends take the samples of the warp with the same tables, mosaics and valid masks."""
    import torch
    from pano360_amd import engine, stitcher, synth
    imgs, rots, intrs = synth.make_scene(n, 32, 24, step_deg=step_deg, seed=seed, kind="A")
    plan = eng.upload_plan(engine.Plan([im.shape[:2] for im in imgs], rots, intrs, False, 1400))
    hits = block_hits(plan.rects, plan.shape)
    assert (16 < hits.min() and hits.max() <= OWN_LIST) if n == 260 else hits.min() > OWN_LIST
    frames = eng.upload_frames(imgs)
    gains = 0.7 + 0.06 * ((7 * np.arange(n)) % 11)           # forged: 0.7 .. 1.3, neighbours differ
    luts = torch.from_numpy(engine.gain_tables(gains)).to(eng.device)
    patches = stitcher._download_patches(eng.warp_all(frames, plan, luts=luts)[0])
    plain = stitcher._download_patches(eng.warp_all(frames, plan)[0])
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(patches, plain))
    want_median, want_valid = median_model.median_blend(patches, plan.shape, 0.1)
    want = {True: oracle.linear_blend(patches, plan.shape), False: oracle.no_blend(patches, plan.shape)}

    def same(got, want_mosaic, cols=slice(None)):
        mosaic, valid = got
        return (np.array_equal(mosaic[:, cols].cpu().numpy(), want_mosaic[:, cols])
                and np.array_equal(valid[:, cols].cpu().numpy().astype(bool), want_valid[:, cols]))

    assert same(eng.median_fused(frames, plan, 0.1, luts=luts), want_median)
    for linear in (True, False):
        assert same(eng.blend_fused(frames, plan, linear, luts=luts), want[linear]), linear
        if n == 260:                                          # a strip start that is no multiple of 64
            assert plan.shape[1] == 192
            for strip in ((0, 100), (100, 192)):
                assert same(eng.blend_fused(frames, plan, linear, strip=strip, luts=luts),
                            want[linear], slice(*strip)), (linear, strip)


def test_fused_on_a_subset_of_the_frames(eng, monkeypatch):
    """A rank's share: only the frames whose rectangles meet the strip, with their ids, give the
    strip of the whole; one of them missing is an error before any kernel runs."""
    from pano360_amd import _lib, engine, synth
    imgs, rots, intrs = synth.make_scene(10, 480, 270, sweep_deg=120.0, jitter=0.01, seed=41,
                                         kind="A")
    plan = eng.upload_plan(engine.Plan([im.shape[:2] for im in imgs], rots, intrs, False, 10 ** 9))
    frames = eng.upload_frames(imgs)
    W = plan.shape[1]
    strip = (W // 3 + 5, W // 2)
    ids = [i for i, (_, _, x0, x1) in enumerate(plan.rects) if x0 < strip[1] and x1 > strip[0]]
    assert 1 < len(ids) < len(imgs)
    want, want_valid = eng.median_fused(frames, plan, 0.1, strip=strip)
    got, got_valid = eng.median_fused([frames[i] for i in ids], plan, 0.1, strip=strip, frame_ids=ids)
    cols = slice(*strip)
    assert np.array_equal(got[:, cols].cpu().numpy(), want[:, cols].cpu().numpy())
    assert np.array_equal(got_valid[:, cols].cpu().numpy(), want_valid[:, cols].cpu().numpy())
    assert want_valid[:, cols].any()
    monkeypatch.setattr(eng, "camera_table", lambda *a, **k: pytest.fail("went on to the kernel's arguments"))
    for fused in (lambda f, i: eng.median_fused(f, plan, 0.1, strip=strip, frame_ids=i),
                  lambda f, i: eng.blend_fused(f, plan, True, frame_ids=i, strip=strip)):
        with pytest.raises(_lib.PanoError, match=rf"frames \[{ids[-1]}\] are needed for columns "
                                                 rf"\[{strip[0]}, {strip[1]}\) but are not resident"):
            fused([frames[i] for i in ids[:-1]], ids[:-1])


def test_drop_in_blender(eng, scene_patches):
    import bundle_adj
    from pano360_amd import stitcher
    name = "scene_small_noise"
    g = load_golden(name)
    imgs, rots, intrs, mr = scene_inputs(g)
    shape, patches = scene_patches[name]

    def regions():
        return [bundle_adj.Image(im.copy(), r.copy(), k.copy())
                for im, r, k in zip(imgs, rots, intrs)]
    saved = stitcher.MAX_RESOLUTION, stitcher.GHOST_TOL
    stitcher.MAX_RESOLUTION = mr
    try:
        assert stitcher.GHOST_TOL == 0.1
        got = stitcher.stitch(regions(), stitcher.BLENDERS["median"])
        assert np.array_equal(got, fused(eng, imgs, rots, intrs, mr, 0.1)[0])
        assert np.array_equal(got, median_model.median_blend(patches, shape, 0.1)[0])
        stitcher.GHOST_TOL = 0.02
        got = stitcher.stitch(regions(), stitcher.BLENDERS["median"])
        want, want_valid = median_model.median_blend(patches, shape, 0.02)
        assert np.array_equal(got, want)
        assert not np.array_equal(got, median_model.median_blend(patches, shape, 0.1)[0])
        # the blender protocol with host patches, and the crop (it consumes the valid mask)
        assert np.array_equal(stitcher.stitch(regions(), lambda p, s: stitcher.median_blend(p, s)),
                              want)
        stitcher.GHOST_TOL = 2
        assert np.array_equal(stitcher.stitch(regions(), stitcher.median_blend, crop=True),
                              g["lin_cropped"])
    finally:
        stitcher.MAX_RESOLUTION, stitcher.GHOST_TOL = saved
