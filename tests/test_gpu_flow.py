"""GPU: the local alignment (csrc/flow.hip, ``--local-align``) against tests/flow_model.py on the
forged patches of tests/flow_cases.py.  Every stage - grey and validity levels, block vectors of
every level, smoothed vectors, output planes, the two pixel counts - is compared for equality;
tests/test_flow_host.py shows on the CPU that the forged cases catch five faults."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flow_cases as fc  # noqa: E402
import flow_model as fm  # noqa: E402

pytestmark = pytest.mark.gpu

# the forged cases, and two planted scenes that reach the levels 3 and 4 (overlaps of 391 and 520)
NAMES = fc.CASES + ("planted-3", "planted-4")


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "planted-3":
        return fc.planted(3, (-15, 15))
    if name == "planted-4":
        img = fc.scene(520, 524, 41)
        rect = (0, 0, 520, 524)
        return ((fc.patch(fc.cut(img, rect), 0, 0), fc.patch(fc.cut(img, rect, (21, -9)), 0, 0)),
                (520, 524), fm.Params(4))
    return fc.case(name)


@functools.lru_cache(maxsize=None)
def model_of(name):
    patches, shape, params = case(name)
    return fm.align(list(patches), shape, params, want_stages=True)


def params_of(p):
    from pano360_amd import flow
    return flow.FlowParams(p.levels, p.gain, p.min_overlap)


def upload(eng, patches, n_blur=0):
    from pano360_amd import stitcher
    return stitcher._upload_patches(eng, list(patches), n_blur)


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    wrong = np.argwhere(got != want)
    if len(wrong):
        first = [tuple(int(v) for v in w) + (got[tuple(w)].item(), want[tuple(w)].item()) for w in wrong[:12]]
        print(f"{what}: {len(wrong)} cells differ; first (index, got, want): {first}")
    assert len(wrong) == 0, what


def words(planes):
    """A patch's float planes as their bit patterns (NaN-proof equality)."""
    return np.ascontiguousarray(planes).view(np.uint32)


def planes_of(dp):
    return dp.planes[:, :, :dp.w].permute(1, 2, 0).contiguous().cpu().numpy()


def model_level(stages, c, level, box):
    g, v = stages["pyramids"][c][level]
    y0, x0, rows, cols = box
    full = g.astype(np.uint16) | (v.astype(np.uint16) << 8)
    out = np.zeros((rows, cols), np.uint16)
    part = full[y0:y0 + rows, x0:x0 + cols]
    out[:part.shape[0], :part.shape[1]] = part
    return out


@pytest.mark.parametrize("name", NAMES)
def test_every_stage_equals_the_model(eng, name):
    from pano360_amd import flow
    patches, shape, params = case(name)
    _, want = model_of(name)
    dev = upload(eng, patches)
    pairs, fields, got = flow.fields_device(dev, shape, params_of(params), eng, want_stages=True)
    assert pairs == want["pairs"]
    rects = [fm.rect_of(p) for p in patches]
    paired = {c for p in pairs for c in p[:2]}
    top = max(p[2] for p in pairs)
    assert set(got["pyramid"]) == {(c, l) for c in paired for l in range(top + 1)}
    for (c, level), plane in got["pyramid"].items():
        assert_same(plane, model_level(want, c, level, fm.box_of(rects[c], level)), f"{name}: camera {c} level {level}")
    assert set(got["vectors"]) == {(q, l) for q, p in enumerate(pairs) for l in range(p[2] + 1)}
    for (q, level), vec in got["vectors"].items():
        assert_same(vec, want["levels"][q][level], f"{name}: pair {q} level {level} vectors")
    for q, f in enumerate(fields):
        assert_same(f, want["fields"][q], f"{name}: pair {q} smoothed")


def raw_align(eng, dev, shape, params, fill):
    """One ``pano_flow_align`` on a workspace filled with ``fill``: (planes per patch or None,
    pyramid, vectors, fields, stats) as host bytes."""
    import torch
    from pano360_amd import engine, flow
    table = engine.patch_table(dev, eng)
    lay = flow.Layout(flow.rects_of(dev), params)
    work = torch.full((lay.total,), fill, dtype=torch.uint8, device=eng.device)
    outs = [torch.full_like(p.planes, 7.0) if lay.paired[c] else None for c, p in enumerate(dev)]
    ptrs = np.array([0 if t is None else t.data_ptr() for t in outs], np.uint64)
    u8 = dict(dtype=torch.uint8, device=eng.device)
    stage = [torch.full((max(n, 1),), 0x55, **u8) for n in (lay.pyramid_bytes, lay.vectors_bytes, lay.fields_bytes)]
    stats = torch.full((4,), -1, dtype=torch.int32, device=eng.device)
    native = params.native()
    eng.call("pano_flow_align", table.host, table.n, shape[0], shape[1], C.byref(native), work, lay.total,
             ptrs, *stage, stats)
    return ([None if t is None else t[:, :, :p.w].cpu().numpy().tobytes() for t, p in zip(outs, dev)],
            [t.cpu().numpy().tobytes() for t in stage], stats.cpu().numpy())


@pytest.mark.parametrize("name", NAMES)
def test_the_whole_stage_equals_the_model(eng, name):
    """``align_device``: planes, masks, statistics; a patch without a pair is the object that
    came in; a second call and a workspace of 0xFF give the same bytes."""
    from pano360_amd import flow
    patches, shape, params = case(name)
    want, stages = model_of(name)
    dev = upload(eng, patches)
    mine = params_of(params)
    aligned, stats = flow.align_device(dev, shape, mine, eng)
    paired = {c for p in stages["pairs"] for c in p[:2]}
    for c, (a, d) in enumerate(zip(aligned, dev)):
        assert a.mask is d.mask and a.blurred is d.blurred and a.scratch is d.scratch and a.rect == d.rect
        assert (a is d) == (c not in paired)
        assert_same(words(planes_of(a)), words(want[c][0]), f"{name}: planes of patch {c}")
        assert_same(d.mask.cpu().numpy().astype(bool), np.asarray(patches[c][1]), f"{name}: mask {c}")
        assert_same(words(planes_of(d)), words(patches[c][0]), f"{name}: the input of patch {c}")
        if a.pitch != a.w:
            assert not a.planes[:, :, a.w:].any()
    moved = sum(int(m.sum()) for m in stages["moved"])
    valid = sum(int((~np.asarray(patches[c][1])).sum()) for c in paired)
    print(f"{name}: {stats}")
    assert (stats["pairs"], stats["moved"], stats["valid"]) == (len(stages["pairs"]), moved, valid)
    known = sum(int(lv[0][..., 2].sum()) for lv in stages["levels"])
    assert stats["known"] == known and stats["blocks"] == sum(lv[0][..., 2].size for lv in stages["levels"])
    first = raw_align(eng, dev, shape, mine, 0x00)
    again = raw_align(eng, dev, shape, mine, 0xFF)
    assert first[0] == again[0] and first[1] == again[1] and np.array_equal(first[2], again[2])
    assert first[0] == [None if c not in paired else np.ascontiguousarray(
        np.moveaxis(want[c][0], 2, 0)).tobytes() for c in range(len(dev))]
    assert first[2].tolist() == [moved, valid, 0, 0]


def test_search_and_smoothing_on_a_forged_pyramid(eng):
    """The stages read what lies in the workspace: random grey, random validity (three quarters
    valid), which no patch produces - the search and the smoothing equal the model on them."""
    import torch
    from pano360_amd import engine, flow
    patches, shape, params = case("three-130x257")
    dev = upload(eng, patches)
    mine = params_of(params)
    table = engine.patch_table(dev, eng)
    lay = flow.Layout(flow.rects_of(dev), mine)
    rng = np.random.default_rng(77)
    host = np.full(lay.total, 0xEE, np.uint8)
    Hp, Wp = 144, 272
    pyr = {}
    for (c, level), (_, rows, cols, y0, x0) in lay.gv.items():
        g = rng.integers(0, 256, (rows, cols)).astype(np.uint16)
        v = (rng.random((rows, cols)) < 0.75).astype(np.uint16)
        lay.level_of(host, c, level)[:] = g | (v << 8)
        full_g, full_v = np.zeros((Hp >> level, Wp >> level), np.uint8), np.zeros((Hp >> level, Wp >> level), bool)
        full_g[y0:y0 + rows, x0:x0 + cols], full_v[y0:y0 + rows, x0:x0 + cols] = g, v.astype(bool)
        pyr.setdefault(c, {})[level] = (full_g, full_v)
    work = torch.from_numpy(host).to(eng.device)
    native = mine.native()
    for stage in ("pano_flow_search", "pano_flow_smooth"):
        eng.call(stage, table.host, table.n, shape[0], shape[1], C.byref(native), work, lay.total)
    got = work.cpu().numpy()
    for q, pair in enumerate(lay.pairs):
        levels = fm.search([pyr[pair[0]][l] for l in range(lay.top + 1)], [pyr[pair[1]][l] for l in range(lay.top + 1)],
                           pair, params, want_levels=True)
        for level, want in enumerate(levels):
            assert_same(lay.vectors_of(got, q, level), want, f"pair {q} level {level}")
        assert_same(lay.field_of(got, q), fm.smooth(levels[0]), f"pair {q} smoothed")
    assert got[:lay.pyramid_bytes].tobytes() == host[:lay.pyramid_bytes].tobytes()


def test_apply_on_forged_vectors(eng):
    """``pano_flow_apply`` alone on smoothed vectors a test wrote: random vectors in -6 .. 6."""
    import torch
    from pano360_amd import engine, flow
    patches, shape, params = case("swapped-130x257")
    dev = upload(eng, patches)
    mine = params_of(params)
    table = engine.patch_table(dev, eng)
    lay = flow.Layout(flow.rects_of(dev), mine)
    rng = np.random.default_rng(78)
    host = np.zeros(lay.total, np.uint8)
    fields = []
    for q in range(len(lay.pairs)):
        f = lay.field_of(host, q)
        f[:] = rng.integers(-6, 7, f.shape)
        fields.append(f.copy())
    work = torch.from_numpy(host).to(eng.device)
    outs = [torch.zeros_like(p.planes) for p in dev]
    stats = torch.zeros(4, dtype=torch.int32, device=eng.device)
    native = mine.native()
    eng.call("pano_flow_apply", table.host, table.n, shape[0], shape[1], C.byref(native), work, lay.total,
             np.array([t.data_ptr() for t in outs], np.uint64), stats)
    moved = 0
    for c, patch in enumerate(patches):
        dx, dy = fm.displacement(list(patches), c, lay.pairs, fields)
        want, mv = fm.warp_patch(patch, dx, dy)
        moved += int(mv.sum())
        got = outs[c][:, :, :dev[c].w].permute(1, 2, 0).contiguous().cpu().numpy()
        assert_same(words(got), words(want), f"patch {c}")
    assert moved > 10000 and stats.cpu().numpy().tolist()[0] == moved


def test_refusals_write_nothing(eng):
    import torch
    from pano360_amd import _lib, engine, flow
    patches, shape, params = case("four-67x300")
    dev = upload(eng, patches)
    mine = params_of(params)
    table = engine.patch_table(dev, eng)
    lay = flow.Layout(flow.rects_of(dev), mine)
    work = torch.full((lay.total,), 0xA5, dtype=torch.uint8, device=eng.device)
    outs = [torch.full_like(p.planes, 3.0) for p in dev]
    ptrs = np.array([t.data_ptr() for t in outs], np.uint64)
    stats = torch.full((4,), -3, dtype=torch.int32, device=eng.device)
    H, W = shape

    def call(table_host=table.host, n=table.n, H=H, W=W, levels=3, gain=16, min_overlap=64, work=work,
             nbytes=lay.total, ptrs=ptrs):
        native = _lib.FlowParams(levels, gain, min_overlap, 0)
        eng.call("pano_flow_align", table_host, n, H, W, C.byref(native), work, nbytes, ptrs, None, None, None, stats)
    windowed = table.host.copy()
    windowed["vh"][1] -= 1
    unmasked = table.host.copy()
    unmasked["mask"][3] = 0
    own = ptrs.copy()
    own[2] = dev[2].planes.data_ptr()
    none = ptrs.copy()
    none[1] = 0
    for bad in (dict(levels=5), dict(levels=-1), dict(gain=0), dict(gain=4081), dict(min_overlap=8), dict(n=1),
                dict(table_host=None), dict(work=None), dict(nbytes=lay.total - 1), dict(W=W - 1), dict(H=0),
                dict(table_host=windowed), dict(table_host=unmasked), dict(ptrs=own), dict(ptrs=none),
                dict(ptrs=None)):
        with pytest.raises(_lib.PanoError):
            call(**bad)
    for stage in ("pano_flow_pyramid", "pano_flow_search", "pano_flow_smooth"):
        with pytest.raises(_lib.PanoError):
            eng.call(stage, table.host, table.n, H, W, C.byref(_lib.FlowParams(9, 16, 64, 0)), work, lay.total)
    assert bool((work == 0xA5).all()) and all(bool((t == 3.0).all()) for t in outs)
    assert stats.cpu().numpy().tolist() == [-3] * 4
    call()                                              # ... and the same call goes through
    assert stats.cpu().numpy().tolist()[2:] == [0, 0] and not bool((work == 0xA5).all())
    assert bool((outs[0] == 3.0).all())                 # patch 0 has no pair: its planes are not written
    # no pair at all: nothing is launched, the patches are the objects that came in
    aligned, st = flow.align_device(dev[:2], shape, mine, eng)
    assert aligned[0] is dev[0] and aligned[1] is dev[1] and st["pairs"] == 0 and st["moved"] == 0


# ------------------------------------------------------------------------ the stitch
@pytest.fixture(scope="module")
def rig(eng):
    """Four frames of 160 x 240 of one panorama, rendered with jittered cameras and registered
    with the unjittered ones: something to align in every overlap."""
    from pano360_amd import synth
    pano = synth.make_frame(5, 1024, 512, "B")
    rots, intrs = synth.make_cameras(4, 240, 160, sweep_deg=90.0)
    shaken, _ = synth.make_cameras(4, 240, 160, sweep_deg=90.0, jitter=0.012, seed=3)
    imgs = [f.cpu().numpy() for f in synth.render_rig(pano, shaken, intrs, 240, 160, eng.device)]
    return imgs, rots, intrs


def regions_of(rig):
    import bundle_adj
    imgs, rots, intrs = rig
    return [bundle_adj.Image(im.copy(), r.copy(), k.copy()) for im, r, k in zip(imgs, rots, intrs)]


_aligned = {}


def model_aligned(eng, rig, padded):
    """The rig's warped patches aligned by the MODEL (once per plan), and the plan."""
    from pano360_amd import engine, stitcher
    if padded not in _aligned:
        imgs, rots, intrs = rig
        plan = eng.upload_plan(engine.Plan([im.shape[:2] for im in imgs], rots, intrs, padded,
                                           stitcher.MAX_RESOLUTION))
        patches, _ = eng.warp_all(eng.upload_frames(imgs), plan)
        host = stitcher._download_patches(patches)
        out, stages = fm.align(host, plan.shape, fm.Params(), want_stages=True)
        assert len(stages["pairs"]) == 3 and sum(int(m.sum()) for m in stages["moved"]) > 5000
        _, valid = eng.ownership(engine.patch_table(patches, eng), plan.shape)
        _aligned[padded] = (out, plan, eng.crop_rect(valid))
    return _aligned[padded]


@pytest.mark.parametrize("crop", (False, True))
@pytest.mark.parametrize("blend", ("none", "linear", "multiband", "median", "seam"))
def test_stitch_with_local_align(eng, rig, blend, crop):
    from pano360_amd import flow, stitcher
    blender = stitcher.BLENDERS[blend]
    banded = blend in ("multiband", "seam")
    got = stitcher.stitch(regions_of(rig), blender, crop=crop, local_align=flow.FlowParams())
    host, plan, rect = model_aligned(eng, rig, banded)
    dev = upload(eng, host, 4 if banded else 0)
    if blend == "multiband":
        want = eng.multiband(dev, plan.shape, 5)[0]
    elif blend == "seam":
        want = eng.seam_multiband(dev, plan.shape, 5, stitcher.SEAM_RATIO)[0]
    elif blend == "median":
        want = eng.median_blend(dev, plan.shape, stitcher.GHOST_TOL)
    else:
        want = eng.simple_blend(dev, plan.shape, linear=blend == "linear")
    want = want.cpu().numpy()
    plain = stitcher._stitch_device(regions_of(rig), blender, False, crop)
    if crop:
        y0, x0, h, w = rect
        assert tuple(plain[1]) == tuple(rect) and (h, w) != tuple(plan.shape)
        want = want[y0:y0 + h, x0:x0 + w]
    assert got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()
    # without the flag the stitch is what it was: the fused stitch's bytes for the fused blenders
    before = stitcher._download_cropped(*plain)
    assert before.shape == got.shape and not np.array_equal(before, got)
    assert stitcher.stitch(regions_of(rig), blender, crop=crop).tobytes() == before.tobytes()
    if blend != "seam" and not crop:
        imgs, _, _ = rig
        fused = eng.stitch(eng.upload_frames(imgs), plan, blend, 5, shortcut=not stitcher.EXACT,
                           **({"tol": stitcher.GHOST_TOL} if blend == "median" else {}))[0]
        assert before.tobytes() == fused.cpu().numpy().tobytes()


def test_a_custom_blender_gets_the_aligned_patches(eng, rig):
    from pano360_amd import flow, stitcher
    host, plan, _ = model_aligned(eng, rig, False)
    seen = {}

    def blender(patches, shape):
        seen["patches"], seen["shape"] = patches, shape
        return stitcher.no_blend(patches, shape)
    got = stitcher.stitch(regions_of(rig), blender, local_align=flow.FlowParams())
    assert tuple(seen["shape"]) == tuple(plan.shape) and len(seen["patches"]) == len(host)
    for (a, ma, ra), (b, mb, rb) in zip(seen["patches"], host):
        assert ra == rb and np.array_equal(ma, mb) and words(a).tobytes() == words(b).tobytes()
    assert got.tobytes() == stitcher.stitch(regions_of(rig), stitcher.no_blend,
                                            local_align=flow.FlowParams()).tobytes()
