"""CPU: the NumPy float32 model of the collapse (tests/compose_model.py) is the reference's - bit
for bit the oracle's multiband_blend on the golden scenes - and the forged cases of
tests/compose_cases.py are well-formed and reach what they were forged for."""
import numpy as np
import pytest

import compose_cases as cc
import compose_model as cm
from conftest import SCENES, load_golden, scene_inputs
from pano360_amd.engine import PATCH_DTYPE

ORACLE_LEVELS = (1, 2, 5, 6)


# ---- 1. the model is the reference's ------------------------------------------------------------
@pytest.fixture(scope="module", params=SCENES)
def scene(request, oracle):
    """The oracle's warped patches, ownership, validity and blurred copies of a golden scene."""
    g = load_golden(request.param)
    imgs, rots, intrs, mr = scene_inputs(g)
    plan, patches, _ = oracle.warp_all(imgs, rots, intrs, True, mr)
    owner = oracle.ownership(patches, plan.shape)
    valid = oracle.valid(patches, plan.shape)
    blurs = []
    for i, (warped, _, ir) in enumerate(patches):
        sharp = warped.copy()
        sharp[..., 3] = owner[ir] == i                                  # stitcher.py:207-208
        blurs.append([oracle.gaussian_blur(sharp, 0, float(np.sqrt(2 * k + 1.0) * 4))
                      for k in range(max(ORACLE_LEVELS) - 1)])
    return request.param, plan.shape, patches, owner, valid, blurs


def whole_patch_case(patches, blurs, n_levels):
    """Records with A = V = the patch and the two arenas, from interleaved host patches."""
    rec = np.zeros(len(patches), PATCH_DTYPE)
    vblocks, ablocks = [], []
    for i, (warped, _, ir) in enumerate(patches):
        h, w = warped.shape[:2]
        pitch = cc.up4(w)
        for key, val in dict(y0=ir[0].start, x0=ir[1].start, h=h, w=w, vh=h, vw=w, ah=h, aw=w,
                             vpitch=pitch, apitch=pitch, index=i).items():
            rec[i][key] = val
        v = np.full((3, h, pitch), cc.GUARD, np.float32)
        v[..., :w] = warped[..., :3].transpose(2, 0, 1)
        vblocks.append(v)
        a = np.full((n_levels - 1, 4, h, pitch), cc.GUARD, np.float32)
        for k in range(n_levels - 1):
            a[k, :, :, :w] = blurs[i][k].transpose(2, 0, 1)
        ablocks.append(a)
    planes, voff, _ = cc.pack(vblocks)
    blurred, aoff, _ = cc.pack(ablocks)
    rec["planes"], rec["blurred"] = voff, aoff
    return rec, planes, blurred


@pytest.mark.parametrize("n_levels", ORACLE_LEVELS)
def test_model_equals_the_oracle_bit_for_bit(oracle, scene, n_levels):
    name, shape, patches, owner, valid, blurs = scene
    rec, planes, blurred = whole_patch_case(patches, blurs, n_levels)
    got_f, got_u8 = cm.collapse(rec, planes, blurred, owner, valid, shape, (0, shape[1]), n_levels)
    fresh = [(w.copy(), m, ir) for w, m, ir in patches]     # the blend overwrites the alphas
    ref_u8, ref_f = oracle.multiband_blend(fresh, shape, n_levels, return_float=True)
    assert got_f.dtype == np.float32 and got_u8.dtype == np.uint8
    assert np.array_equal(got_f.view(np.uint32), ref_f.view(np.uint32)), (name, n_levels)
    assert np.array_equal(got_u8, ref_u8), (name, n_levels)


def test_model_produces_the_strip_only():
    c = cc.case("overlap", 3)
    args = (c["records"], c["planes"], c["blurred"], c["owner"], c["valid"], c["shape"])
    full_f, full_u8 = cm.collapse(*args, (0, 203), 3)
    for xs0, xs1 in cc.STRIPS:
        f, u8 = cm.collapse(*args, (xs0, xs1), 3)
        assert np.array_equal(f[:, xs0:xs1], full_f[:, xs0:xs1])
        assert np.array_equal(u8[:, xs0:xs1], full_u8[:, xs0:xs1])
        assert not f[:, :xs0].any() and not f[:, xs1:].any()
        assert not u8[:, :xs0].any() and not u8[:, xs1:].any()


# ---- 2. the cases reach what they are for -------------------------------------------------------
def model_stats(c):
    stats = {}
    W = c["shape"][1]
    cm.collapse(c["records"], c["planes"], c["blurred"], c["owner"], c["valid"], c["shape"],
                (0, W), c["n_levels"], stats=stats)
    return stats


# per case and level (L >= 2); `many` is its whole table - the cuts only choose the kernel's path
REACH = [p for p in cc.compose_params() if p[0] == "overlap" or p == ("many", cc.MANY_LEVELS, 300)]


@pytest.mark.parametrize("p", REACH, ids=cc.param_id)
def test_case_reaches_its_paths(p):
    """Conditions on the model over the pixels of the full strip; asserted, so that a later edit
    of the cases cannot empty them."""
    c = cc.get(p)
    s = model_stats(c)
    H, W = c["shape"]
    assert s["zero"].mean() >= 0.01, ("weight sum 0 under a record", s["zero"].mean())
    low, high = (s["raw"] < 0).any(axis=2), (s["raw"] > 1).any(axis=2)
    assert low.mean() >= 0.01 and high.mean() >= 0.01, ("clipped", low.mean(), high.mean())
    assert (s["m"] >= 3).mean() >= 0.05, ("three records", (s["m"] >= 3).mean())
    for r in c["records"]:           # first and last row and column of every A are on the mosaic
        ys, xs = cm.area(r)
        assert 0 <= ys.start < ys.stop <= H and 0 <= xs.start < xs.stop <= W


def test_overlap_geometry():
    c = cc.case("overlap", 2)
    rec = c["records"]
    assert len(rec) == 7
    areas = [cm.area(r) for r in rec]
    m = model_stats(c)["m"]
    assert m.max() == 5 and (m == 5).sum() >= 40
    sizes = {(ys.stop - ys.start, xs.stop - xs.start) for ys, xs in areas}
    assert {(1, 1), (1, 40), (30, 1)} <= sizes
    col_edges = {xs.start for _, xs in areas} | {xs.stop - 1 for _, xs in areas}
    row_edges = {ys.start for ys, _ in areas} | {ys.stop - 1 for ys, _ in areas}
    assert {0, 63, 64, 65, 127, 128, 202} <= col_edges
    assert {0, 3, 4, 36} <= row_edges
    # two records share an index, with disjoint rectangles
    same = [(i, j) for i in range(7) for j in range(i + 1, 7) if rec[i]["index"] == rec[j]["index"]]
    assert same
    for i, j in same:
        (ya, xa), (yb, xb) = areas[i], areas[j]
        assert (ya.stop <= yb.start or yb.stop <= ya.start or xa.stop <= xb.start
                or xb.stop <= xa.start)
    assert any(r["vx0"] > 0 and r["vy0"] > 0 and r["ax0"] > r["vx0"] for r in rec)
    # the one-level case is the same geometry and its owner map names every index and "none"
    one = cc.case("one_level", 1)
    for key in PATCH_DTYPE.names:
        if key not in ("planes", "blurred"):
            assert np.array_equal(one["records"][key], rec[key]), key
    assert set(np.unique(one["owner"])) == {-1} | set(int(v) for v in rec["index"])


def test_many_meets_three_ballot_masks_in_one_wave_row():
    c = cc.case("many", cc.MANY_LEVELS)
    rec = c["records"]
    assert len(rec) == 300 == cc.MANY_CUTS[-1]
    ah, aw = rec["ah"], rec["aw"]
    assert ah.min() == 3 and ah.max() == 9 and aw.min() == 5 and aw.max() == 11
    H, W = c["shape"]
    best = 0
    for y in range(H):
        for wx0 in range(0, W, 64):
            groups = set()
            for i in range(256):
                ys, xs = cm.area(rec[i])
                if ys.start <= y < ys.stop and xs.start < min(wx0 + 64, W) and xs.stop > wx0:
                    groups.add(i // 64)
            best = max(best, len(groups))
    assert best >= 3, best


def test_empty_case():
    for lv in cc.LEVELS:
        c = cc.case("empty", lv)
        assert len(c["records"]) == 0
        f, u8 = cm.collapse(c["records"], c["planes"], c["blurred"], c["owner"], c["valid"],
                            c["shape"], (0, 203), lv)
        assert not f.any() and not u8.any()


# ---- 3. structure -------------------------------------------------------------------------------
@pytest.mark.parametrize("p", cc.compose_params(), ids=cc.param_id)
def test_case_structure(p):
    c = cc.get(p)
    assert c["shape"] == cc.SHAPE == (37, 203)
    check_structure(c, cc.case(p[0], p[1])["records"])


@pytest.mark.parametrize("n_levels", cc.RIG_LEVELS)
def test_rig_case_structure(n_levels):
    """The `overlap` records scaled to the mosaic of the rig the interior pixels are checked on
    (the plan is host geometry) obey the same rules, and still overlap."""
    from pano360_amd import engine
    imgs, rots, intrs, cap = cc.rig_scene()
    shape = engine.Plan([im.shape[:2] for im in imgs], rots, intrs, True, cap).shape
    assert 64 < shape[1] <= 400
    c = cc.rig_case(shape, n_levels)
    check_structure(c, c["records"])
    m = model_stats(c)["m"]
    assert len(c["records"]) == 7 and m.max() == 5 and (m >= 3).mean() >= 0.05
    assert (m == 0).any() and (m == 1).any()


def check_structure(c, full):
    """``c``: a case; ``full``: the whole table its arenas were packed for."""
    H, W = c["shape"]
    rec, L = c["records"], c["n_levels"]
    assert rec.dtype == PATCH_DTYPE
    i32 = lambda r, k: int(r[k])    # noqa: E731
    for r in rec:
        y0, x0, h, w = (i32(r, k) for k in ("y0", "x0", "h", "w"))
        vy0, vx0, vh, vw = (i32(r, k) for k in ("vy0", "vx0", "vh", "vw"))
        ay0, ax0, ah, aw = (i32(r, k) for k in ("ay0", "ax0", "ah", "aw"))
        assert 0 <= y0 and 0 <= x0 and h > 0 and w > 0 and y0 + h <= H and x0 + w <= W
        assert 0 <= vy0 and 0 <= vx0 and vy0 + vh <= h and vx0 + vw <= w         # V in the patch
        assert vy0 <= ay0 and vx0 <= ax0 and ah > 0 and aw > 0                   # A in V
        assert ay0 + ah <= vy0 + vh and ax0 + aw <= vx0 + vw
        assert vx0 % 4 == 0 and ((vx0 + vw) % 4 == 0 or vx0 + vw == w)
        assert r["vpitch"] % 4 == 0 and r["vpitch"] >= vw
        assert r["apitch"] % 4 == 0 and r["apitch"] >= aw
    # the blocks and the guard runs tile the arenas, in table order
    for arena, guards, key, size in (
            (c["planes"], c["guards_planes"], "planes", lambda r: 3 * int(r["vh"]) * int(r["vpitch"])),
            (c["blurred"], c["guards_blurred"], "blurred",
             lambda r: (L - 1) * 4 * int(r["ah"]) * int(r["apitch"]))):
        assert arena.dtype == np.float32 and np.isfinite(arena).all()
        assert len(guards) == len(full) + 1
        at = 0
        for k, (a, b) in enumerate(guards):
            assert a == at and b - a == cc.GUARD_FLOATS == 64
            assert (arena[a:b] == cc.GUARD).all()
            at = b
            if k < len(full):
                assert int(full[k][key]) == at
                at += size(full[k])
        assert at == arena.size
    # values: colours in [-0.5, 1.5], alphas from the set, a tenth of `valid` is 0
    for i in range(len(rec)):
        v = cm.window(rec, c["planes"], i)
        vw, aw = int(rec[i]["vw"]), int(rec[i]["aw"])
        assert v[..., :vw].min() >= -0.5 and v[..., :vw].max() <= 1.5
        assert (v[..., vw:] == cc.GUARD).all()
        if L > 1:
            b = cm.copies(rec, c["blurred"], i, L - 1)
            assert b[:, :3, :, :aw].min() >= -0.5 and b[:, :3, :, :aw].max() <= 1.5
            assert np.isin(b[:, 3, :, :aw], cc.ALPHAS).all()
            assert (b[..., aw:] == cc.GUARD).all()
    assert 0.05 <= (c["valid"] == 0).mean() <= 0.15
    assert c["owner"].dtype == np.int16 and c["valid"].dtype == np.uint8
