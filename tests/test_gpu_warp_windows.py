"""GPU: the window warp alone (pano_warp_windows, csrc/warp.hip) on the rigs and forged window
tables of tests/warp_cases.py.  The whole-patch warp of every rig is first held to the oracle
bit for bit (maps, mask, RGBA planes); every window must then be, by bits, the crop of its
patch's whole-patch colour planes, and nothing else of the arena may be written.  Every
comparison is exact."""
import numpy as np
import pytest

import warp_cases as wc

pytestmark = pytest.mark.gpu

NAN_BITS = wc.NAN_BITS


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module", params=wc.RIGS)
def rig(request, eng):
    """A rig on the device with its whole-patch warps (shared and per-camera colour tables)."""
    import torch
    from pano360_amd import engine
    r = wc.rig(request.param)
    plan = eng.upload_plan(wc.make_plan(engine.Plan, r))
    frames = eng.upload_frames(r["imgs"])
    patches, maps = eng.warp_all(frames, plan, want_maps=True)
    gains = np.linspace(0.7, 1.3, plan.n)
    luts = torch.from_numpy(engine.gain_tables(gains)).to(eng.device)
    tinted, _ = eng.warp_all(frames, plan, luts=luts)
    colour = lambda ps: [p.planes[:3, :, :p.w].cpu().numpy() for p in ps]      # noqa: E731
    return dict(name=request.param, host=r, plan=plan, frames=frames, patches=patches, maps=maps,
                cams=eng.camera_table(plan, dict(enumerate(frames))), luts=luts,
                ref={"shared": colour(patches), "percam": colour(tinted)})


def test_whole_patch_warp_is_the_oracles(eng, oracle, rig):
    """Pins the reference of the windows below: maps, mask and RGBA planes bit for bit."""
    r, plan = rig["host"], rig["plan"]
    oplan = wc.make_plan(oracle.Plan, r)
    assert oplan.shape == plan.shape and list(oplan.rects) == list(plan.rects)
    for i, (dp, (mx, my)) in enumerate(zip(rig["patches"], rig["maps"])):
        shape = r["imgs"][i].shape[:2]
        omx, omy, omask = oracle.inverse_map(oplan.projs[i], oplan, plan.rects[i], shape)
        assert np.array_equal(bits(mx.cpu().numpy()), bits(omx)), (rig["name"], i)
        assert np.array_equal(bits(my.cpu().numpy()), bits(omy)), (rig["name"], i)
        assert np.array_equal(dp.mask.cpu().numpy().astype(bool), omask), (rig["name"], i)
        want = oracle.remap(oracle.add_weights(r["imgs"][i]), omx, omy)
        want[..., 3] *= ~omask
        got = dp.planes[:, :, :dp.w].permute(1, 2, 0).contiguous().cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (rig["name"], i)


def test_windows_reach_both_tap_paths(eng, rig):
    """Judged on the whole-patch maps the test above ties to the oracle (the CPU suite judges
    the same on the oracle's maps): windows wholly inside their frame and windows with pixels
    of both kinds."""
    win = Windows(eng, rig)
    maps = [tuple(m.cpu().numpy() for m in pair) for pair in rig["maps"]]
    whole, mixed = wc.windows_by_taps(win.rec, maps, [im.shape[:2] for im in rig["host"]["imgs"]])
    assert whole >= 1 and mixed >= 1, (rig["name"], whole, mixed)


class Windows:
    """The forged table of a rig on the device, its arena prefilled with NAN_BITS."""

    def __init__(self, eng, rig, seed=7):
        import torch
        from pano360_amd import engine
        self.eng, self.rig = eng, rig
        self.rec, self.floats = wc.windows(rig["plan"].rects, rig["plan"].centres, seed)
        self.arena = torch.full((self.floats,), NAN_BITS, dtype=torch.int32, device=eng.device)
        rec = self.rec.copy()
        rec["planes"] = self.arena.data_ptr() + 4 * self.rec["planes"]
        self.table = engine.PatchTable(rec, eng)                # tiles_off, extents, upload
        assert self.table.max_vw == self.rec["vw"].max() and self.table.max_vh == self.rec["vh"].max()

    def call(self, which="shared", need=None):
        """One warp into a freshly prefilled arena; the arena's bits on the host."""
        self.arena.fill_(NAN_BITS)
        lut, stride = (self.eng.lut255, 0) if which == "shared" else (self.rig["luts"], 256)
        t = self.table
        self.eng.call("pano_warp_windows", self.rig["cams"], t.dev, t.n, t.max_vw, t.max_vh,
                      *self.rig["plan"].dev, lut, stride, need)
        return self.arena.cpu().numpy().view(np.uint32)

    def blocks(self, arena):
        """Per record: (record with tiles_off, its [3][vh][vpitch] block of ``arena``)."""
        for k, r in enumerate(self.table.host):
            off, vh, vp = int(self.rec[k]["planes"]), int(r["vh"]), int(r["vpitch"])
            yield k, r, arena[off:off + 3 * vh * vp].reshape(3, vh, vp)

    def expected(self, which):
        """The arena when every window is written: crops of the whole-patch planes, NAN_BITS
        in the guard floats and the pitch padding."""
        want = np.full(self.floats, NAN_BITS, np.uint32)
        for k, r, block in self.blocks(want):
            vy0, vx0, vh, vw = (int(r[key]) for key in ("vy0", "vx0", "vh", "vw"))
            ref = self.rig["ref"][which][int(r["index"])]
            block[:, :, :vw] = bits(ref[:, vy0:vy0 + vh, vx0:vx0 + vw])
        return want

    def explain(self, got, want):
        for k, r, block in self.blocks(got != want):
            if block.any():
                c, y, x = (int(v) for v in np.argwhere(block)[0])
                return (f"record {k} (camera {int(r['index'])}, V = {int(r['vy0'])}, {int(r['vx0'])}, "
                        f"{int(r['vh'])} x {int(r['vw'])}): {int(block.sum())} floats differ, first at "
                        f"plane {c}, row {y}, column {x}")
        return f"{int((got != want).sum())} guard floats were written"


@pytest.mark.parametrize("which", ["shared", "percam"])
def test_windows_are_crops_of_the_whole_patch(eng, rig, which):
    win = Windows(eng, rig)
    rec = win.rec
    assert len(rec) == 4 * rig["plan"].n
    want = win.expected(which)
    assert not (want == NAN_BITS).all() and (want[:wc.GUARD_FLOATS] == NAN_BITS).all()
    got = win.call(which)
    assert np.array_equal(got, want), (rig["name"], which, win.explain(got, want))
    again = win.call(which)
    assert np.array_equal(again, got), (rig["name"], which, "a second call differs")


def needed_pixels(r, need):
    """bool [vh][vw]: the pixels of V whose 32 x 32 tile (grid of rectangle A, clamped) is
    flagged in ``need`` - stated per pixel, without any block size."""
    ax0, ay0, aw, ah = (int(r[k]) for k in ("ax0", "ay0", "aw", "ah"))
    ntx = ((ax0 + aw - 1) >> 5) - (ax0 >> 5) + 1
    nty = ((ay0 + ah - 1) >> 5) - (ay0 >> 5) + 1
    ys = np.clip(((int(r["vy0"]) + np.arange(int(r["vh"]))) >> 5) - (ay0 >> 5), 0, nty - 1)
    xs = np.clip(((int(r["vx0"]) + np.arange(int(r["vw"]))) >> 5) - (ax0 >> 5), 0, ntx - 1)
    tiles = need[int(r["tiles_off"]):int(r["tiles_off"]) + ntx * nty].reshape(nty, ntx)
    return tiles[ys][:, xs] != 0, (nty, ntx)


def test_need_flags(eng, rig):
    import torch
    assert eng.tile_grid == 32
    win = Windows(eng, rig)
    want = win.expected("shared")
    plain = win.call("shared")
    host = win.table.host
    n_tiles = win.table.n_tiles
    forged = {"all": np.ones(n_tiles, np.uint8), "none": np.zeros(n_tiles, np.uint8),
              "checkerboard": np.zeros(n_tiles, np.uint8), "single": np.zeros(n_tiles, np.uint8)}
    most = 0
    for k, r in enumerate(host):
        _, (nty, ntx) = needed_pixels(r, forged["none"])
        board = (np.add.outer(np.arange(nty), np.arange(ntx)) & 1).astype(np.uint8)
        forged["checkerboard"][int(r["tiles_off"]):int(r["tiles_off"]) + nty * ntx] = board.ravel()
        if nty * ntx > most:
            most, single_at = nty * ntx, int(r["tiles_off"]) + (nty * ntx) // 2
    forged["single"][single_at] = 1
    assert most >= 4
    for label, need in forged.items():
        got = win.call("shared", need=torch.from_numpy(need).to(eng.device))
        written = got != NAN_BITS
        assert np.array_equal(got[written], want[written]), (rig["name"], label, "a written float is wrong")
        for k, r, block in win.blocks(written):
            needed, _ = needed_pixels(r, need)
            missing = needed[None] & ~block[:, :, :int(r["vw"])]
            assert not missing.any(), (rig["name"], label, "record", k, "needed pixel not written",
                                       np.argwhere(missing)[0].tolist())
        if label == "all":
            assert np.array_equal(got, plain), (rig["name"], "all tiles needed differs from need = NULL")


def test_refusals_write_nothing(eng, rig):
    from pano360_amd import _lib
    win = Windows(eng, rig)
    t, plan = win.table, rig["plan"]
    bad = {
        "n = 65536": (rig["cams"], t.dev, 65536, t.max_vw, t.max_vh, *plan.dev, eng.lut255, 0, None),
        "null table": (rig["cams"], None, t.n, t.max_vw, t.max_vh, *plan.dev, eng.lut255, 0, None),
        "negative lut_stride": (rig["cams"], t.dev, t.n, t.max_vw, t.max_vh, *plan.dev, eng.lut255,
                                -256, None),
    }
    win.arena.fill_(NAN_BITS)
    for label, args in bad.items():
        with pytest.raises(_lib.PanoError) as err:
            eng.call("pano_warp_windows", *args)
        assert f"({_lib.EINVAL})" in str(err.value), (label, str(err.value))
        assert (win.arena.cpu().numpy().view(np.uint32) == NAN_BITS).all(), label
