"""GPU: the collapse alone (pano_multiband_compose, csrc/blend.hip) on the forged record tables
of tests/compose_cases.py, bit for bit against the NumPy float32 model of tests/compose_model.py
(which tests/test_compose_host.py ties to the oracle, bit for bit).  Every comparison is exact.

Per case x level x strip: float and uint8 inside the strip equal the model as numbers, the uint8
is trunc(255 * the kernel's own float), nothing outside the strip and nothing of the arenas is
written, mosaic_f32 = NULL and a second run give the same bytes.  Interior pixels are checked on
a real tiny rig with a forged interior map against the owner's whole-patch warp."""
import numpy as np
import pytest

import compose_cases as cc
import compose_model as cm

pytestmark = pytest.mark.gpu

U8_FILL = 0xA5
NAN_BITS = 0x7FC5A5A5           # a quiet NaN nothing computes


class Device:
    """A case on the device: arenas, owner, valid and the table with addresses in it."""

    def __init__(self, eng, case):
        import torch
        self.eng, self.case = eng, case
        up = lambda a: torch.from_numpy(np.array(a)).to(eng.device)     # noqa: E731
        self.planes, self.blurred = up(case["planes"]), up(case["blurred"])
        self.owner, self.valid = up(case["owner"]), up(case["valid"])
        rec = case["records"].copy()
        rec["planes"] = self.planes.data_ptr() + 4 * case["records"]["planes"]
        rec["blurred"] = self.blurred.data_ptr() + 4 * case["records"]["blurred"]
        self.n = len(rec)
        self.table = up((rec if self.n else np.zeros(1, rec.dtype)).view(np.uint8))  # never null
        self.shape = case["shape"]

    def outputs(self, want_float=True):
        import torch
        H, W = self.shape
        u8 = torch.full((H, W, 3), U8_FILL, dtype=torch.uint8, device=self.eng.device)
        fl = None
        if want_float:
            fl = torch.full((H, W, 3), NAN_BITS, dtype=torch.int32, device=self.eng.device)
        return u8, fl

    def run(self, strip, n_levels=None, want_float=True, interior=None, classes=None, cams=None,
            tabs=(None, None, None), lut=None, lut_stride=0, out=None):
        """One call; (uint8 [H][W][3], float32 bits as uint32 [H][W][3] or None) on the host."""
        H, W = self.shape
        u8, fl = out or self.outputs(want_float)
        self.eng.call("pano_multiband_compose", self.table, self.n, H, W, strip[0], strip[1],
                      self.case["n_levels"] if n_levels is None else n_levels, self.owner,
                      self.valid, interior, classes, cams, *tabs,
                      self.eng.lut255 if lut is None else lut, lut_stride, u8, fl)
        return u8.cpu().numpy(), None if fl is None else fl.cpu().numpy().view(np.uint32)

    def arenas_unchanged(self):
        return (np.array_equal(self.planes.cpu().numpy().view(np.uint32),
                               self.case["planes"].view(np.uint32))
                and np.array_equal(self.blurred.cpu().numpy().view(np.uint32),
                                   self.case["blurred"].view(np.uint32)))


def first_difference(got, want, xs0, records, what):
    """None, or a message naming the first differing (y, x, c) of two strips that start at mosaic
    column xs0 and the records over it."""
    bad = np.argwhere(got != want)
    if not len(bad):
        return None
    y, x, c = (int(v) for v in bad[0])
    over = cm.records_over(records, y, xs0 + x)
    return (f"{what}: {len(bad)} values differ, first at (y={y}, x={xs0 + x}, c={c}): got "
            f"{got[y, x, c]!r}, model {want[y, x, c]!r}; records over it (table positions) {over}")


def check_strip(got_u8, got_bits, want_f, want_u8, strip, records, label):
    """The strip equals the model as numbers, the bytes are the kernel's own floats truncated,
    and everything outside the strip kept its prefill."""
    xs0, xs1 = strip
    got_f = got_bits.view(np.float32)
    inside = np.s_[:, xs0:xs1]
    assert not np.isnan(got_f[inside]).any(), (label, "a pixel of the strip was not written")
    msg = first_difference(got_f[inside], want_f[inside], xs0, records, "float")
    assert msg is None, (label, strip, msg)
    msg = first_difference(got_u8[inside], want_u8[inside], xs0, records, "uint8")
    assert msg is None, (label, strip, msg)
    own = (np.float32(255) * got_f[inside]).astype(np.uint8)
    assert np.array_equal(got_u8[inside], own), (label, strip)
    for outside in (np.s_[:, :xs0], np.s_[:, xs1:]):
        assert (got_u8[outside] == U8_FILL).all(), (label, strip)
        assert (got_bits[outside] == NAN_BITS).all(), (label, strip)


# ---- 1. bit for bit against the model; nothing else is written -----------------------------------
@pytest.mark.parametrize("p", cc.compose_params(), ids=cc.param_id)
def test_collapse_equals_the_model(eng, p):
    case = cc.get(p)
    dev = Device(eng, case)
    H, W = case["shape"]
    model = lambda strip: cm.collapse(case["records"], case["planes"], case["blurred"],   # noqa: E731
                                      case["owner"], case["valid"], (H, W), strip, case["n_levels"])
    for strip in cc.STRIPS:
        want_f, want_u8 = model(strip)
        got_u8, got_bits = dev.run(strip)
        check_strip(got_u8, got_bits, want_f, want_u8, strip, case["records"], cc.param_id(p))
        if p[0] == "empty":
            assert not got_u8[:, strip[0]:strip[1]].any() and not got_bits[:, strip[0]:strip[1]].any()
        only_u8, _ = dev.run(strip, want_float=False)
        assert np.array_equal(only_u8, got_u8), (p, strip, "mosaic_f32 = NULL changes the bytes")
        again_u8, again_bits = dev.run(strip)
        assert np.array_equal(again_u8, got_u8) and np.array_equal(again_bits, got_bits), (p, strip)
    assert dev.arenas_unchanged(), p


# ---- 2. interior pixels, on a real tiny rig ------------------------------------------------------
@pytest.fixture(scope="module")
def rig(eng):
    """3 noise frames of 64 x 48, 25 degrees apart: plan, cameras, real owner / valid, a forged
    interior map and the whole-patch warps (shared and per-camera colour tables)."""
    import torch
    from pano360_amd import engine
    imgs, rots, intrs, cap = cc.rig_scene()
    plan = eng.upload_plan(engine.Plan([im.shape[:2] for im in imgs], rots, intrs, True, cap))
    frames = eng.upload_frames(imgs)
    cams = eng.camera_table(plan, dict(enumerate(frames)))
    owner_d, valid_d = eng.ownership_cameras(plan, cams=cams)
    owner, valid = owner_d.cpu().numpy(), valid_d.cpu().numpy()
    H, W = plan.shape
    ib = eng.interior_block
    assert ib == 4
    H8, W8 = -(-H // ib), -(-W // ib)
    # blocks whose 16 pixels are all owned; a seeded half of them is "interior"
    full = np.zeros((H8, W8), bool)
    two = np.zeros((H8, W8), bool)
    for by in range(H // ib):
        for bx in range(W // ib):
            blk = owner[by * ib:(by + 1) * ib, bx * ib:(bx + 1) * ib]
            full[by, bx] = (blk >= 0).all()
            two[by, bx] = full[by, bx] and len(np.unique(blk)) >= 2
    rng = np.random.default_rng(5)
    interior = (full & (rng.random((H8, W8)) < 0.5)).astype(np.uint8)
    assert (interior != 0).sum() >= 20 and ((interior != 0) & two).sum() >= 2, \
        ("the forged interior map needs blocks with two owners", int(((interior != 0) & two).sum()))
    gains = np.linspace(0.7, 1.3, plan.n)
    luts = torch.from_numpy(engine.gain_tables(gains)).to(eng.device)
    warps = {}
    for key, tables in (("shared", None), ("percam", luts)):
        patches, _ = eng.warp_all(frames, plan, luts=tables)
        warps[key] = [p.planes[:3, :, :p.w].cpu().numpy() for p in patches]
    return dict(plan=plan, frames=frames, cams=cams, owner=owner, valid=valid, interior=interior,
                luts=luts, warps=warps, shape=(H, W))


def rig_case(rig, n_levels):
    c = dict(cc.rig_case(rig["shape"], n_levels))
    c["owner"], c["valid"] = rig["owner"], rig["valid"]
    return c


def expected_on_rig(rig, case, strip, which):
    """The model, with the owner's whole-patch warped colour on the pixels of interior blocks."""
    H, W = rig["shape"]
    want_f, _ = cm.collapse(case["records"], case["planes"], case["blurred"], case["owner"],
                            case["valid"], (H, W), strip, case["n_levels"])
    inner = np.repeat(np.repeat(rig["interior"] != 0, 4, axis=0), 4, axis=1)[:H, :W]
    inner[:, :strip[0]], inner[:, strip[1]:] = False, False
    for y, x in np.argwhere(inner):
        o = int(rig["owner"][y, x])
        y0, _, x0, _ = rig["plan"].rects[o]
        v = rig["warps"][which][o][:, y - y0, x - x0]
        assert (v >= 0).all() and (v <= 1).all()
        want_f[y, x] = v
    return want_f, (np.float32(255) * want_f).astype(np.uint8), inner


@pytest.mark.parametrize("which", ["shared", "percam"])
@pytest.mark.parametrize("n_levels", cc.RIG_LEVELS)
def test_interior_pixels_are_the_owners_warp(eng, rig, n_levels, which):
    case = rig_case(rig, n_levels)
    dev = Device(eng, case)
    H, W = rig["shape"]
    import torch
    interior = torch.from_numpy(rig["interior"]).to(eng.device)
    lut, stride = (None, 0) if which == "shared" else (rig["luts"], 256)
    for strip in ((0, W), (5, W - 3)):
        want_f, want_u8, inner = expected_on_rig(rig, case, strip, which)
        got_u8, got_bits = dev.run(strip, interior=interior, cams=rig["cams"], tabs=rig["plan"].dev,
                                   lut=lut, lut_stride=stride)
        got_f = got_bits.view(np.float32)
        where = np.argwhere(inner[..., None] & (got_f != want_f))
        assert not len(where), ("interior pixel is not the owner's warp", which, n_levels,
                                where[0].tolist(), len(where))
        check_strip(got_u8, got_bits, want_f, want_u8, strip, case["records"], (which, n_levels))
        again_u8, again_bits = dev.run(strip, interior=interior, cams=rig["cams"],
                                       tabs=rig["plan"].dev, lut=lut, lut_stride=stride)
        assert np.array_equal(again_u8, got_u8) and np.array_equal(again_bits, got_bits)
    assert dev.arenas_unchanged()


def test_level_class_option_changes_nothing_when_classes_are_zero(eng, rig):
    import torch
    from pano360_amd import _lib
    case = rig_case(rig, 4)
    dev = Device(eng, case)
    H, W = rig["shape"]
    interior = torch.from_numpy(rig["interior"]).to(eng.device)
    classes = torch.zeros_like(interior)
    kw = dict(interior=interior, cams=rig["cams"], tabs=rig["plan"].dev)
    off = dev.run((0, W), classes=classes, **kw)
    assert eng.get_option(_lib.OPT_LEVEL_CLASSES) == 0
    eng.set_option(_lib.OPT_LEVEL_CLASSES, 1)
    try:
        on = dev.run((0, W), classes=classes, **kw)
    finally:
        eng.set_option(_lib.OPT_LEVEL_CLASSES, 0)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    want_f, want_u8, _ = expected_on_rig(rig, case, (0, W), "shared")
    check_strip(on[0], on[1], want_f, want_u8, (0, W), case["records"], "classes 0")


# ---- 3. refusals ---------------------------------------------------------------------------------
def test_refusals_leave_the_prefill(eng):
    import torch
    from pano360_amd import _lib
    case = cc.case("overlap", 3)
    dev = Device(eng, case)
    H, W = case["shape"]
    classes = torch.zeros((-(-H // 4), -(-W // 4)), dtype=torch.uint8, device=eng.device)
    bad = {
        "n_levels 0": dict(strip=(0, W), n_levels=0),
        "n_levels 9": dict(strip=(0, W), n_levels=9),
        "xs1 > W": dict(strip=(0, W + 1)),
        "classes without interior": dict(strip=(0, W), classes=classes),
        "lut_stride 7": dict(strip=(0, W), lut_stride=7),
    }
    for label, kw in bad.items():
        out = dev.outputs()
        with pytest.raises(_lib.PanoError) as err:
            dev.run(out=out, **kw)
        assert f"({_lib.EINVAL})" in str(err.value), (label, str(err.value))
        torch.cuda.synchronize()
        assert (out[0].cpu().numpy() == U8_FILL).all(), label
        assert (out[1].cpu().numpy().view(np.uint32) == NAN_BITS).all(), label
    assert dev.arenas_unchanged()
