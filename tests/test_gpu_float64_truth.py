"""GPU: the multiband blend per pixel against the float64 restatement (tests/multiband_f64.py).

Every case compares the kernels' blurred planes or float mosaic with the float64 truth at every
compared pixel, in units of the pixel's own error scale (e = |got - truth| / (u s)), and checks:

1. the kernel's e <= E, the bound the restatement derives from the arithmetic;
2. the float32 oracle, on the same pixels, is within E too (the bound is not tuned to the GPU);
3. the kernel's worst e is at most 4 x the oracle's worst e on the same pixels.

The truth starts from the oracle's float32 warped patches, which the GPU warp matches bit for bit,
so the comparison isolates the blur and collapse arithmetic.
"""
import numpy as np
import pytest

import multiband_f64 as mf
from conftest import SCENES, load_golden, scene_inputs

pytestmark = pytest.mark.gpu

RATIO = 4.0


def _judge(tag, e_got, e_ref, E):
    got, ref = float(np.max(e_got)), float(np.max(e_ref))
    print(f"{tag}: kernel worst e {got:.3f}, oracle worst e {ref:.3f}, E {E:.1f}")
    assert ref <= E, (tag, "oracle", ref, E)
    assert got <= E, (tag, "kernel", got, E)
    assert got <= RATIO * ref, (tag, "ratio", got, ref)
    return got, ref


# ------------------------------------------------------------------ a. blurred planes
_RECTS = [(0, 63, 0, 97), (10, 75, 40, 135), (5, 36, 90, 219), (0, 97, 150, 183),
          (30, 42, 20, 220), (0, 120, 200, 210), (50, 55, 60, 67), (20, 129, 100, 131)]


def _synthetic_records(eng, n_blur, seed):
    """Whole-patch records of 32k +- 1 columns and rows, and ones narrower or lower than the
    radius (12 rows, 10 columns, 5 x 7), over one mosaic, filled with seeded [0, 1] colour."""
    import torch
    from pano360_amd import engine
    rng = np.random.default_rng(seed)
    H = max(r[1] for r in _RECTS)
    W = max(r[3] for r in _RECTS)
    patches, host = [], []
    for rect in _RECTS:
        dp = engine.DevicePatch(rect, eng.device, n_blur)
        h, w = dp.h, dp.w
        rgba = rng.random((h, w, 4)).astype(np.float32)
        rgba[..., 3] = rgba[..., 3] * 0.9 + 0.05
        planes = np.zeros((4, h, dp.pitch), np.float32)
        planes[:, :, :w] = rgba.transpose(2, 0, 1)
        dp.planes.copy_(torch.from_numpy(planes))
        dp.mask.zero_()
        patches.append(dp)
        host.append((rgba, np.zeros((h, w), bool), np.s_[rect[0]:rect[1], rect[2]:rect[3]]))
    return patches, host, (H, W)


@pytest.mark.parametrize("blur", ["mfma", "valu"])
@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("levels", [2, 5, 6, 8])
def test_blurred_planes_against_float64(oracle, blur, lean, levels):
    """Every level's four blurred planes of ragged and narrow records (apertures 33 to 117 taps:
    one and two levels per workgroup, both group sizes) against the float64 blur."""
    from pano360_amd import _lib, engine
    eng = engine.Engine(blur=blur)
    eng.set_option(_lib.OPT_BLUR_LEAN, lean)
    n_blur = levels - 1
    patches, host, shape = _synthetic_records(eng, n_blur, 700 + levels)
    table = engine.patch_table(patches, eng)
    owner, valid = eng.ownership(table, shape)
    eng.blur_and_compose(table, owner, valid, shape, levels)
    own = mf.ownership_f64(host, shape)
    assert np.array_equal(owner.cpu().numpy().astype(np.int32), own)
    sig = engine.level_sigmas(levels)
    e_got, e_ref = [], []
    for i, (dp, (rgba, _, ir)) in enumerate(zip(patches, host)):
        sharp = rgba.copy()
        sharp[..., 3] = own[ir] == i
        got = dp.blurred[:, :, :, :dp.w].cpu().numpy()
        for k, s in enumerate(sig):
            n = engine.gaussian_ksize(s)
            truth = mf.blur_f64(sharp, s)
            ref = oracle.gaussian_blur(sharp, n, s)
            e_got.append(mf.plane_error(got[k].transpose(1, 2, 0), truth, n).max())
            e_ref.append(mf.plane_error(ref, truth, n).max())
    _judge(f"planes {blur} lean={lean} L={levels}", e_got, e_ref,
           mf.plane_bound(mf.max_taps(levels)))


@pytest.mark.parametrize("blur", ["mfma", "valu"])
def test_windowed_blurred_planes_against_float64(oracle, blur):
    """The fused path's records (windows V, rectangles A cut from the patches, tiles anchored at
    multiples of 32): the blurred copies over A against the float64 blur of the whole patch."""
    import torch
    from pano360_amd import engine, synth
    eng = engine.Engine(blur=blur)
    imgs, rots, intrs = synth.make_scene(6, 640, 360, sweep_deg=50.0, jitter=0.01, seed=31, kind="A")
    plan = engine.Plan([im.shape[:2] for im in imgs], rots, intrs, True, 10 ** 9)
    _, _, _, fused = eng.stitch(eng.upload_frames(imgs), plan, "multiband", 5, shortcut=False)
    torch.cuda.synchronize()
    _, ref_patches, _ = oracle.warp_all(imgs, rots, intrs, True, 10 ** 9)
    own = mf.ownership_f64(ref_patches, plan.shape)
    sig = engine.level_sigmas(5)
    arena, base = fused.blurred, fused.blurred.data_ptr()
    truth, ref = {}, {}
    e_got, e_ref = [], []
    for rec in fused.table.host:
        idx, ah, aw, ap = int(rec["index"]), int(rec["ah"]), int(rec["aw"]), int(rec["apitch"])
        ay0, ax0 = int(rec["ay0"]), int(rec["ax0"])
        off = (int(rec["blurred"]) - base) // 4
        got = arena[off:off + 4 * 4 * ah * ap].view(4, 4, ah, ap)[:, :, :, :aw].cpu().numpy()
        if idx not in truth:
            warped, _, ir = ref_patches[idx]
            sharp = warped.copy()
            sharp[..., 3] = own[ir] == idx
            truth[idx] = [mf.blur_f64(sharp, s) for s in sig]
            ref[idx] = [oracle.gaussian_blur(sharp, engine.gaussian_ksize(s), s) for s in sig]
        for k, s in enumerate(sig):
            n = engine.gaussian_ksize(s)
            t = truth[idx][k][ay0:ay0 + ah, ax0:ax0 + aw]
            e_got.append(mf.plane_error(got[k].transpose(1, 2, 0), t, n).max())
            e_ref.append(mf.plane_error(ref[idx][k][ay0:ay0 + ah, ax0:ax0 + aw], t, n).max())
    _judge(f"windowed planes {blur}", e_got, e_ref, mf.plane_bound(mf.max_taps(5)))


# ------------------------------------------------------------------ b. float mosaic
def _check_mosaic(oracle, tag, patches, shape, levels, got_f):
    """Kernel float mosaic ``got_f`` (whole mosaic of ``shape``) and the oracle's against the truth
    of the oracle's float32 ``patches``."""
    truth, s, overlap = mf.multiband_f64(patches, shape, levels)
    copies = [(w.copy(), m, ir) for w, m, ir in patches]     # (the oracle overwrites the alphas)
    _, ref_f = oracle.multiband_blend(copies, shape, levels, return_float=True)
    e_got = mf.normalised_error(got_f, truth, s)
    e_ref = mf.normalised_error(ref_f, truth, s)
    return _judge(tag, e_got, e_ref, mf.bound(mf.max_taps(levels), levels, overlap))


def _stitch_and_check(eng, oracle, tag, imgs, rots, intrs, mr, levels, **kw):
    from pano360_amd import engine
    plan = engine.Plan([im.shape[:2] for im in imgs], rots, intrs, True, mr)
    _, fl, _, _ = eng.stitch(eng.upload_frames(imgs), plan, "multiband", levels, want_float=True,
                             **kw)
    _, patches, _ = oracle.warp_all(imgs, rots, intrs, True, mr)
    return _check_mosaic(oracle, tag, patches, plan.shape, levels, fl.cpu().numpy())


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("levels", [1, 2, 5, 6, 8])
def test_golden_scenes_float_mosaic_against_float64(eng, oracle, name, levels):
    imgs, rots, intrs, mr = scene_inputs(load_golden(name))
    _stitch_and_check(eng, oracle, f"{name} L={levels}", imgs, rots, intrs, mr, levels)


def _degenerate(case):
    from pano360_amd import synth
    if case == "single":
        return synth.make_scene(1, 200, 120, sweep_deg=0.0, seed=1, kind="B")
    if case == "disjoint":
        return synth.make_scene(2, 160, 100, step_deg=75.0, seed=2, kind="B")
    if case == "tiny":
        return synth.make_scene(3, 24, 14, sweep_deg=50.0, jitter=0.01, seed=3, kind="A")
    return synth.make_scene(4, 90, 260, sweep_deg=40.0, jitter=0.01, seed=4, kind="B")


@pytest.mark.parametrize("case", ["single", "disjoint", "tiny", "tall"])
def test_degenerate_scenes_against_float64(eng, oracle, case):
    imgs, rots, intrs = _degenerate(case)
    for levels in (2, 5):
        _stitch_and_check(eng, oracle, f"{case} L={levels}", imgs, rots, intrs, 10 ** 9, levels)


@pytest.mark.parametrize("shortcut", [True, False])
@pytest.mark.parametrize("classes", [0, 1])
@pytest.mark.parametrize("kind", ["A", "B"])
def test_interior_shortcut_and_level_classes_against_float64(oracle, shortcut, classes, kind):
    """The interior shortcut on and off, the level-class collapse on and off, L = 5 and 3."""
    from pano360_amd import _lib, engine, synth
    eng = engine.Engine()
    eng.set_option(_lib.OPT_LEVEL_CLASSES, classes)
    imgs, rots, intrs = synth.make_scene(6, 640, 360, sweep_deg=50.0, jitter=0.01, seed=33,
                                         kind=kind)
    for levels in (5, 3):
        _stitch_and_check(eng, oracle, f"shortcut={shortcut} classes={classes} {kind} L={levels}",
                          imgs, rots, intrs, 10 ** 9, levels, shortcut=shortcut)


def test_closed_360_sweep_against_float64(eng, oracle):
    from pano360_amd import engine, synth
    n, w, h = 24, 160, 90
    imgs, rots, intrs = synth.make_scene(n, w, h, step_deg=15.0, jitter=0.004, seed=77, kind="B",
                                         n_levels=6)
    plan = engine.Plan([(h, w)] * n, rots, intrs, True, 10 ** 9)
    assert max(r[3] - r[2] for r in plan.rects) > 0.9 * plan.shape[1]     # seam-straddling frames
    _stitch_and_check(eng, oracle, "closed 360 L=6", imgs, rots, intrs, 10 ** 9, 6)


@pytest.mark.parametrize("world", [3, 8])
def test_column_strips_against_float64(eng, oracle, world):
    """Each rank's strip (only its frames resident) against the truth on the strip's columns."""
    from pano360_amd import dist as pdist
    from pano360_amd import engine, synth
    imgs, rots, intrs = synth.make_scene(10, 480, 270, sweep_deg=120.0, jitter=0.01, seed=41,
                                         kind="A")
    shapes = [im.shape[:2] for im in imgs]
    _, patches, _ = oracle.warp_all(imgs, rots, intrs, True, 10 ** 9)
    plan0 = engine.Plan(shapes, rots, intrs, True, 10 ** 9)
    fl = np.zeros(plan0.shape + (3,), np.float32)
    for rank in range(world):
        st = pdist.ShardedStitcher(eng, shapes, rots, intrs, 5, rank, world, exchange=None)
        plan = engine.Plan(shapes, rots, intrs, True, 10 ** 9, table_cols=st.table_cols)
        eng.upload_plan(plan)
        _, f, _, _ = eng.multiband_fused(eng.upload_frames([imgs[i] for i in st.my_frames]), plan,
                                         5, want_float=True, frame_ids=st.my_frames, strip=st.strip)
        c0, c1 = st.strip
        fl[:, c0:c1] = f[:, c0:c1].cpu().numpy()
    _check_mosaic(oracle, f"strips world={world}", patches, plan0.shape, 5, fl)


def test_other_paths_against_float64(oracle):
    """The whole-patch stage path, the launch-by-launch fused path, and trusted / kept-geometry
    repeats (bit-identical to the default elsewhere; one case each)."""
    from pano360_amd import engine, synth
    imgs, rots, intrs = synth.make_scene(5, 320, 180, sweep_deg=70.0, jitter=0.01, seed=43, kind="B")
    plan = engine.Plan([im.shape[:2] for im in imgs], rots, intrs, True, 10 ** 9)
    _, patches, _ = oracle.warp_all(imgs, rots, intrs, True, 10 ** 9)
    eng = engine.Engine()
    frames = eng.upload_frames(imgs)
    _, f, _, _ = eng.stitch(frames, plan, "multiband", 6, want_float=True, fused=False)
    _check_mosaic(oracle, "whole-patch path L=6", patches, plan.shape, 6, f.cpu().numpy())
    loose = engine.Engine()
    loose.native_stitch = False
    _, f, _, _ = loose.stitch(frames, plan, "multiband", 6, want_float=True)
    _check_mosaic(oracle, "launch by launch L=6", patches, plan.shape, 6, f.cpu().numpy())
    for keep in (False, True):
        kept = engine.Engine().trust_layouts(True, keep_geometry=keep)
        for _ in range(3):
            _, f, _, _ = kept.stitch(frames, plan, "multiband", 6, want_float=True)
        kept.verify_trusted()
        _check_mosaic(oracle, f"trusted keep_geometry={keep} L=6", patches, plan.shape, 6,
                      f.cpu().numpy())


def test_equalised_scene_with_gains_above_one_against_float64(eng, oracle):
    """Frames of one scene at very different brightness: the gains of the equalisation reach well
    above 1.  The gain tables clip to [0, 1] as stitcher.py:66 does, so the blur's inputs stay in
    the range MB_IN_SCALE assumes, but dark frames brought up by a gain fill that range with values
    off the 1/255 grid.  The truth starts from the warp of the frames through the engine's gain
    tables (the oracle's remap of the same float32 RGBA)."""
    from pano360_amd import engine, synth
    imgs, rots, intrs = synth.make_scene(4, 320, 200, sweep_deg=60.0, jitter=0.01, seed=8, kind="B")
    imgs = [np.clip(im.astype(np.float64) * f, 0, 255).astype(np.uint8)
            for im, f in zip(imgs, (1.0, 0.35, 0.8, 0.3))]
    frames = eng.upload_frames(imgs)
    _, _, gains, luts = eng.equalize_gains(frames, rots, intrs)
    assert np.max(gains) > 1.2 and np.max(gains) > 3.0 * np.min(gains), gains
    plan = engine.Plan([im.shape[:2] for im in imgs], rots, intrs, True, 10 ** 9)
    eng.upload_plan(plan)
    lut = luts.cpu().numpy()
    oplan = oracle.Plan([im.shape[:2] for im in imgs], rots, intrs, True, 10 ** 9)
    patches = []
    for i, (img, proj, rect) in enumerate(zip(imgs, oplan.projs, oplan.rects)):
        rgba = oracle.add_weights(img)
        rgba[..., :3] = lut[i][img]
        mx, my, mask = oracle.inverse_map(proj, oplan, rect, img.shape[:2])
        warped = oracle.remap(rgba, mx, my)
        warped[..., 3][mask] = 0.0
        patches.append((warped, mask, np.s_[rect[0]:rect[1], rect[2]:rect[3]]))
    assert max(float(p[0][..., :3].max()) for p in patches) <= 1.0
    for levels in (5, 8):
        _, f, _, _ = eng.stitch(frames, plan, "multiband", levels, want_float=True, luts=luts)
        _check_mosaic(oracle, f"equalised L={levels}", patches, plan.shape, levels, f.cpu().numpy())


# ------------------------------------------------------------------ c. full size, distinct frames
class _RolledFrames:
    """Camera i's frame = roll(base[i % k], (a i, b i)), made on the host only when indexed.  Only
    the latest frame is kept (``_oracle_window`` uses each camera once per window: index, convert,
    move on), and iterating yields shape holders, so nothing is rolled for the plan."""

    class _Shape:
        def __init__(self, shape):
            self.shape = shape

    def __init__(self, host, n, a, b):
        self.host, self.n, self.a, self.b, self.latest = host, n, a, b, (None, None)

    def __len__(self):
        return self.n

    def __iter__(self):
        return (self._Shape(self.host[i % len(self.host)].shape) for i in range(self.n))

    def __getitem__(self, i):
        if self.latest[0] != i:
            # (made while the previous frame is still referenced, so the two never share an id)
            frame = np.roll(self.host[i % len(self.host)], (self.a * i, self.b * i), (0, 1))
            self.latest = (i, frame)
        return self.latest[1]


class _LatestOnly(dict):
    """The RGBA cache handed to ``_oracle_window``: it keeps only the entry stored last (an 8K float32
    RGBA image is 530 MB, and a window of config 5 meets 20 - 41 cameras' rectangles)."""

    def __setitem__(self, key, value):
        self.clear()
        super().__setitem__(key, value)


@pytest.mark.parametrize("name", ["cfg3", "cfg5"])
def test_full_size_distinct_frames_against_float64(eng, oracle, name):
    """BASELINE configs 3 and 5 at full size with EVERY camera's frame distinct (frame i = base
    frame i % 2 rolled by (37 i, 53 i)), so a camera that reads a neighbour's frame changes the
    mosaic.  Windows (``_seam_windows``): one on every seam of config 3, so every camera owns
    pixels in some window, and on sixteen seeded seams of config 5 (of 120: a camera of config 5
    is seen only where one of its seams was drawn); both ends of the sweep and a corner.  Compared
    on the window shrunk by the largest radius R.
    The device holds every camera's frame (config 5: about 12 GB); the host rolls and converts one
    camera's frame at a time (under 1 GB), at the cost of converting a full frame for every camera
    whose rectangle meets a window (config 5's seam-straddling frames meet them all)."""
    import torch
    from pano360_amd import engine, synth
    from test_gpu_fullsize import _oracle_window, _seam_windows
    cfg = synth.CONFIGS[name]
    n, w, h, levels = cfg["n"], cfg["width"], cfg["height"], cfg["n_levels"]
    rots, intrs = synth.make_cameras(n, w, h, sweep_deg=cfg.get("sweep_deg"),
                                     step_deg=cfg.get("step_deg"))
    plan = eng.upload_plan(engine.Plan([(h, w)] * n, rots, intrs, True, 10 ** 9))
    H, W = plan.shape
    R = max(engine.gaussian_ksize(s) // 2 for s in engine.level_sigmas(levels))
    owner = eng.ownership_cameras(plan)[0].cpu().numpy()
    S = 288
    windows, pairs, _ = _seam_windows(owner, S, np.random.default_rng(707 + n),
                                      None if name == "cfg3" else 16)
    if name == "cfg3":                  # every camera owns pixels in some window
        assert set(np.unique(pairs).tolist()) == set(range(n))
    del owner
    windows += [(H // 2, H // 2 + S, W - S, W), (H // 2, H // 2 + S, 0, S), (H - S, H, W - S, W)]
    a, b = 37, 53
    host = [synth.make_frame(i, w, h, "B") for i in range(2)]
    base = eng.upload_frames(host)
    frames = [torch.roll(base[i % 2], (a * i, b * i), (0, 1)) for i in range(n)]
    del base
    _, fl, _, _ = eng.stitch(frames, plan, "multiband", levels, want_float=True)
    del frames
    imgs = _RolledFrames(host, n, a, b)
    e_got_all, e_ref_all, bounds = [], [], []
    for win in windows:
        wy0, wy1, wx0, wx1 = win
        _, patches, shape = _oracle_window(oracle, imgs, _LatestOnly(), rots, intrs, True, win)
        iy0, iy1 = (R if wy0 > 0 else 0), (wy1 - wy0) - (R if wy1 < H else 0)
        ix0, ix1 = (R if wx0 > 0 else 0), (wx1 - wx0) - (R if wx1 < W else 0)
        got = fl[wy0:wy1, wx0:wx1].cpu().numpy()
        truth, s, overlap = mf.multiband_f64(patches, shape, levels)
        _, ref_f = oracle.multiband_blend(patches, shape, levels, return_float=True)
        sl = (slice(iy0, iy1), slice(ix0, ix1))
        assert truth[sl].max() > 0
        e_got_all.append(mf.normalised_error(got[sl], truth[sl], s[sl]).max())
        e_ref_all.append(mf.normalised_error(ref_f[sl], truth[sl], s[sl]).max())
        bounds.append(mf.bound(mf.max_taps(levels), levels, max(overlap, 1)))
        assert e_ref_all[-1] <= bounds[-1], (name, win, "oracle", e_ref_all[-1], bounds[-1])
        assert e_got_all[-1] <= bounds[-1], (name, win, "kernel", e_got_all[-1], bounds[-1])
    _judge(f"{name} full size, {len(windows)} windows, distinct frames", e_got_all, e_ref_all,
           min(bounds))
