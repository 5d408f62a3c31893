"""GPU: the seam routing (csrc/seam_route.hip, ``-b seam``) against tests/seam_route_model.py on
the forged inputs of tests/seam_route_cases.py.  Owners, labels and levels are integers and every
comparison of them is equality; tests/test_seam_route_host.py shows on the CPU that the forged
planes catch a flood with 8-connectivity, ``D > d``, reversed groups or no admissibility."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import seam_route_cases as sc  # noqa: E402
import seam_route_model as sm  # noqa: E402

pytestmark = pytest.mark.gpu


def upload(eng, patches, n_blur=0):
    from pano360_amd import engine, stitcher
    dev = stitcher._upload_patches(eng, patches, n_blur)
    return dev, engine.patch_table(dev, eng)


def flood(eng, planes):
    """(owner, label plane after the flood, stats) of one ``pano_seam_route_flood`` call."""
    import torch
    a, second, diff, label, group, n, n_groups = planes
    H, W = label.shape
    dev = [torch.from_numpy(np.ascontiguousarray(p)).to(eng.device) for p in (a, second, diff, label)]
    owner = torch.full((H, W), -7, dtype=torch.int16, device=eng.device)
    stats = torch.full((4,), -1, dtype=torch.int32, device=eng.device)
    eng.call("pano_seam_route_flood", *dev, np.ascontiguousarray(group, np.int32), n, n_groups, H, W,
             owner, stats)
    return owner.cpu().numpy(), dev[3].cpu().numpy(), stats.cpu().numpy()


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    wrong = np.argwhere(got != want)
    if len(wrong):
        first = [tuple(int(v) for v in w) + (int(got[tuple(w)]), int(want[tuple(w)])) for w in wrong[:12]]
        print(f"{what}: {len(wrong)} cells differ; first (index, got, want): {first}")
    assert len(wrong) == 0, what


@pytest.mark.parametrize("name", sc.PATCHES)
def test_prepare_equals_the_model(eng, name):
    import torch
    patches, shape, ratio = sc.PATCHES[name]
    want = sm.prepare(patches, shape, ratio)
    _, table = upload(eng, patches)
    H, W = shape
    owner0, valid = eng.ownership(table, shape)
    assert_same(owner0.cpu().numpy(), want["a"], f"{name}: a")
    assert_same(valid.cpu().numpy().astype(bool), want["valid"], f"{name}: valid")
    i16 = dict(dtype=torch.int16, device=eng.device)
    u8 = dict(dtype=torch.uint8, device=eng.device)
    second, label = torch.full((H, W), -9, **i16), torch.full((H, W), -9, **i16)
    diff, pairs, present = torch.full((H, W), 9, **u8), torch.full((table.n, table.n), 9, **u8), \
        torch.full((256,), 9, **u8)
    eng.call("pano_seam_route_prepare", table.dev, table.n, H, W, owner0, float(ratio), second,
             diff, label, pairs, present)
    for key, got in (("second", second), ("diff", diff), ("label", label), ("pairs", pairs),
                     ("present", present)):
        assert_same(got.cpu().numpy(), want[key], f"{name}: {key}")


@pytest.mark.parametrize("name", sc.PLANES)
def test_flood_equals_the_heap_loop(eng, name):
    """Every label, the owner map, the classes that labelled a cell and the pixels that changed
    owner; a second run gives the same bytes."""
    planes = sc.PLANES[name]
    heap, want, worked = sc.truth(name)
    owner, label, stats = flood(eng, planes)
    print(f"{name} {heap.shape}: classes {stats[0]} (sweep {worked}), rounds {stats[1]}, most in "
          f"one class {stats[2]}, moved {stats[3]}")
    assert_same(label, heap, f"{name}: labels")
    assert_same(owner, want, f"{name}: owner")
    assert int(stats[0]) == worked
    assert int(stats[3]) == int(((want != planes[0]) & (want >= 0)).sum())
    again, label2, stats2 = flood(eng, planes)
    assert owner.tobytes() == again.tobytes() and label.tobytes() == label2.tobytes()
    assert int(stats2[0]) == worked


@pytest.mark.parametrize("name", sc.SERPENTINES)
def test_one_class_outlasts_a_batch_of_rounds(eng, name):
    """Class (255, group of camera 1) carries 1 along the whole corridor: more rounds than the
    host queues between two reads of "done" (PANO_SEAM_BATCH = 64), so a read lands inside the
    class.  The count is the device's own (``stats[2]``) and depends on when tiles load their
    frames: a round moves the label at least one tile on, and every second corridor runs against
    the order the tiles are launched in."""
    owner, _, stats = flood(eng, sc.PLANES[name])
    print(f"{name}: {stats[1]} rounds, {stats[2]} in one class")
    assert int(stats[2]) > sc.BATCH
    assert_same(owner, sc.truth(name)[1], name)


@pytest.mark.parametrize("name", sc.PATCHES)
def test_route_equals_the_model(eng, name):
    """``pano_seam_route``: ownership, prepare, the colouring on the host, the flood."""
    patches, shape, ratio = sc.PATCHES[name]
    want, want_valid, p = sm.route(patches, shape, ratio)
    _, table = upload(eng, patches)
    owner, valid, stats = eng.seam_route(table, shape, ratio)
    stats = stats.cpu().numpy()
    print(f"{name}: classes {stats[0]}, rounds {stats[1]}, most {stats[2]}, moved {stats[3]}, "
          f"open {stats[4]}, groups {stats[5]}")
    assert_same(owner.cpu().numpy(), want, f"{name}: owner")
    assert_same(valid.cpu().numpy().astype(bool), want_valid, f"{name}: valid")
    assert int(stats[3]) == int(((want != p["a"]) & (want >= 0)).sum())
    assert int(stats[4]) == int(p["open"].sum())
    assert int(stats[5]) == p["n_groups"]
    again, _, stats2 = eng.seam_route(table, shape, ratio)
    assert owner.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    assert int(stats2.cpu()[0]) == int(stats[0])


def owner_of(patches, shape):
    """The owner map ``seam_blend`` / ``multiband_blend`` left in the patches' alpha."""
    owner = np.full(shape, -1, np.int16)
    for idx, (warped, _, irange) in enumerate(patches):
        view = owner[irange]
        view[warped[..., 3] == 1] = idx
    return owner


def test_seam_blend_routes_around_what_one_frame_shows(eng):
    import torch
    from pano360_amd import stitcher
    forged, shape, ratio = sc.ghost_pair()
    assert ratio == stitcher.SEAM_RATIO
    want, want_valid, p = sm.route(forged, shape, ratio)
    patches = copy.deepcopy(forged)
    mosaic = stitcher.seam_blend(patches, shape)
    owner = owner_of(patches, shape)
    assert_same(owner, want, "owner")
    # the mosaic is the stage multiband on the model's owner map
    _, table = upload(eng, forged, 4)
    staged, _ = eng.blur_and_compose(table, torch.from_numpy(want).to(eng.device),
                                     torch.from_numpy(want_valid.astype(np.uint8)).to(eng.device),
                                     shape, 5)
    assert mosaic.tobytes() == staged.cpu().numpy().tobytes()
    # the routed seam lies on what both frames show alike, the argmax seam does not
    assert sm.seam_pairs(owner).any() and not p["diff"][sm.seam_pairs(owner)].any()
    plain = copy.deepcopy(forged)
    stitcher.multiband_blend(plain, shape)
    argmax = owner_of(plain, shape)
    assert_same(argmax, p["a"], "argmax owner")
    assert p["diff"][sm.seam_pairs(argmax)].any()
    # a ratio of its own
    narrow = copy.deepcopy(forged)
    stitcher.seam_blend(narrow, shape, ratio=0.9)
    assert_same(owner_of(narrow, shape), sm.route(forged, shape, 0.9)[0], "owner at ratio 0.9")


@pytest.fixture(scope="module")
def rig(eng):
    """Four frames of 160 x 240 looking at one smooth panorama, and something that only the
    second frame shows, in its overlap with the third."""
    from pano360_amd import synth
    pano = synth.make_frame(3, 1024, 512, "B")
    rots, intrs = synth.make_cameras(4, 240, 160, sweep_deg=90.0)
    imgs = [f.cpu().numpy() for f in synth.render_rig(pano, rots, intrs, 240, 160, eng.device)]
    imgs[1][60:100, 150:175] = (250, 20, 230)
    return imgs, rots, intrs


@pytest.mark.parametrize("crop", (False, True))
def test_stitch_with_the_seam_blender(eng, rig, crop):
    import bundle_adj
    from pano360_amd import engine, stitcher
    imgs, rots, intrs = rig

    def regions():
        return [bundle_adj.Image(im.copy(), r.copy(), k.copy()) for im, r, k in zip(imgs, rots, intrs)]
    got = stitcher.stitch(regions(), stitcher.BLENDERS["seam"], crop=crop)
    # the host-patch route: the blender protocol on the downloaded warps
    plan = eng.upload_plan(engine.Plan([im.shape[:2] for im in imgs], rots, intrs, True,
                                       stitcher.MAX_RESOLUTION))
    frames = eng.upload_frames(imgs)
    patches, _ = eng.warp_all(frames, plan)
    host = stitcher._download_patches(patches)
    want = stitcher.seam_blend(host, plan.shape)
    if crop:
        _, valid = eng.ownership(engine.patch_table(patches, eng), plan.shape)
        y0, x0, h, w = eng.crop_rect(valid)
        want = want[y0:y0 + h, x0:x0 + w]
        assert (h, w) != plan.shape
    assert got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()
    if crop:
        return
    # the routing did something here, and multiband is what it was: the fused stitch's bytes,
    # within one level of the stage path's (the fast path's contract, stitcher.EXACT)
    argmax, _ = eng.ownership(engine.patch_table(patches, eng), plan.shape)
    assert (owner_of(host, plan.shape) != argmax.cpu().numpy()).any()
    plain = stitcher.stitch(regions(), stitcher.BLENDERS["multiband"])
    assert not np.array_equal(plain, got)
    fused = eng.stitch(frames, plan, "multiband", 5)[0].cpu().numpy()
    assert plain.tobytes() == fused.tobytes()
    # ... and with every pixel through the full band sum (stitcher.EXACT) it is the stage path's
    # mosaic, byte for byte, on the engine that mode uses
    saved = stitcher.EXACT
    stitcher.EXACT = True
    try:
        exact = stitcher.stitch(regions(), stitcher.BLENDERS["multiband"])
        valu = stitcher._engine_for_stitch()
    finally:
        stitcher.EXACT = saved
    staged = valu.stitch(valu.upload_frames(imgs), plan, "multiband", 5, fused=False)[0].cpu().numpy()
    assert exact.tobytes() == staged.tobytes()
    assert np.abs(plain.astype(int) - staged.astype(int)).max() <= 1
