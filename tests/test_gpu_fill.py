"""GPU: the fill stage (pano360_amd/fill.py, csrc/fill.hip) against its float64 model
(tests/fill_model.py) and against exact properties.

Valid pixels must be the input's bytes.  A hole value must equal the model's unless the model's
f_0 lies within 4e-3 of a half (``fill_model.near_tie``), where it may differ by one level.  Why
4e-3: values are at most 255 and an operation rounds by 2^-24 relative, so a level adds at most
6e-5 (4 operations per pull, 7 per push); over 15 + 15 levels of convex combinations that is below
2.5e-3, and only a value that close to a half can round differently in float32 and float64.  At
most 2 % of a case's hole values are that close (tests/test_fill_host.py).  How many differ is
printed, not asserted.  Everything else here is exact: equalities between device results."""
import ctypes as C

import numpy as np
import pytest
import torch

import fill_cases
import fill_model as fm
import view_cases
from pano360_amd import _lib, fill, tiles, view

pytestmark = pytest.mark.gpu


def _compare(name, got, img, mask, want, f0):
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got[mask != 0], img[mask != 0]), name
    holes = np.broadcast_to((mask == 0)[..., None], want.shape)
    near = fm.near_tie(f0) & holes
    delta = np.abs(got.astype(int) - want.astype(int))
    print(f"{name}: {int(holes.sum())} hole values, {int(near.sum())} near a tie, "
          f"{int((delta != 0).sum())} differ from the model")
    assert not delta[holes & ~near].any(), name
    assert delta[near].max(initial=0) <= 1, name


# --------------------------------------------------------------- against the model
@pytest.mark.parametrize("name", fill_cases.CASES)
def test_fill_equals_the_model(eng, name):
    img, mask, closed, want, f0 = fill_cases.case(name)
    got = fill.fill(img, mask, closed, eng)
    _compare(name, got, img, mask, want, f0)
    if not (mask != 0).any():
        assert np.array_equal(got, img)
    again = fill.fill(img, mask, closed, eng)           # the same bytes on a second call
    assert np.array_equal(again, got)


def test_fill_of_a_crop_view_with_pitches(eng):
    """A rectangle of a larger image and of a larger mask: pitch > 3 w, mask pitch > w."""
    big = fill_cases.noise(90, 150, 21)
    big_mask = fm.blobs(90, 150, 14, 9.0, seed=5)
    dev, dev_mask = torch.from_numpy(big).to(eng.device), torch.from_numpy(big_mask).to(eng.device)
    y0, x0, h, w = 7, 13, 70, 101
    view_img, view_mask = dev[y0:y0 + h, x0:x0 + w], dev_mask[y0:y0 + h, x0:x0 + w]
    assert view_img.stride(0) > 3 * w and view_mask.stride(0) > w
    got = fill.fill_device(view_img, view_mask, False, eng).cpu().numpy()
    img, mask = big[y0:y0 + h, x0:x0 + w], big_mask[y0:y0 + h, x0:x0 + w]
    want, f0 = fm.fill(img, mask)
    _compare("crop view", got, img, mask, want, f0)
    assert np.array_equal(dev.cpu().numpy(), big)       # the source is untouched
    # a bool mask is the same mask
    assert np.array_equal(fill.fill_device(view_img, view_mask != 0, False, eng).cpu().numpy(), got)


@pytest.mark.parametrize("name", ["64x64_tail_alone-noise", "611x1103_closed-noise"])
def test_fill_in_place(eng, name):
    img, mask, closed, want, f0 = fill_cases.case(name)
    fresh = fill.fill(img, mask, closed, eng)
    dev = torch.from_numpy(img.copy()).to(eng.device)
    out = fill.fill_device(dev, mask, closed, eng, out=dev)
    assert out is dev and np.array_equal(dev.cpu().numpy(), fresh)
    # ... and in place inside a larger image: what lies around the rectangle stays
    h, w = img.shape[:2]
    big = torch.full((h + 5, w + 9, 3), 77, dtype=torch.uint8, device=eng.device)
    inner = big[2:2 + h, 4:4 + w]
    inner.copy_(torch.from_numpy(img.copy()))
    fill.fill_device(inner, mask, closed, eng, out=inner)
    host = big.cpu().numpy()
    assert np.array_equal(host[2:2 + h, 4:4 + w], fresh)
    host[2:2 + h, 4:4 + w] = 77
    assert (host == 77).all()


# ------------------------------------------------------------- exact properties
@pytest.mark.parametrize("shape", [(5, 9), (64, 64), (65, 64), (131, 257), (611, 1103)])
def test_exact_properties(eng, shape):
    h, w = shape
    mask = fm.blobs(h, w, 8, max(2.0, min(h, w) / 6), seed=h)
    assert 0 < mask.sum() < mask.size
    const = np.empty((h, w, 3), np.uint8)
    const[:] = (3, 140, 255)
    garbage = np.where(mask[..., None] != 0, const, 99).astype(np.uint8)
    noise = fill_cases.noise(h, w, 17)
    one = np.zeros((h, w), np.uint8)
    one[(2 * h) // 3, w // 5] = 1
    for closed in (False, True):
        assert np.array_equal(fill.fill(garbage, mask, closed, eng), const)
        assert (fill.fill(noise, one, closed, eng) == noise[(2 * h) // 3, w // 5]).all()
        assert np.array_equal(fill.fill(noise, np.zeros_like(mask), closed, eng), noise)
        assert np.array_equal(fill.fill(noise, np.ones_like(mask), closed, eng), noise)


# ------------------------------------------------------------------- the select
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096 + 5, 300 * 301])
def test_select_equals_where(eng, n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, (n, 1, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (n, 1, 3), dtype=np.uint8)
    mask = (rng.integers(0, 3, (n, 1)) * 100).astype(np.uint8)         # 0, 100, 200
    want = np.where(mask[..., None] != 0, a, b)
    da, db, dm = (torch.from_numpy(v).to(eng.device) for v in (a, b, mask))
    assert np.array_equal(fill.select_device(da, dm, db, eng).cpu().numpy(), want)
    # pointers off 16 bytes take the path of one pixel per thread
    pad = torch.zeros(3 * n + 3, dtype=torch.uint8, device=eng.device)
    odd = pad[3:].view(n, 1, 3)
    odd.copy_(da)
    assert np.array_equal(fill.select_device(odd, dm, db, eng).cpu().numpy(), want)
    out = fill.select_device(da, dm, db, eng, out=da)                   # in place
    assert out is da and np.array_equal(da.cpu().numpy(), want)


def test_the_abi_refuses_bad_arguments(eng):
    img = torch.zeros((4, 5, 3), dtype=torch.uint8, device=eng.device)
    mask = torch.ones((4, 5), dtype=torch.uint8, device=eng.device)
    out = torch.empty_like(img)
    p, i64 = _lib._ptr, C.c_int64

    def call(img_p=p(img), pitch=15, mask_p=p(mask), mpitch=5, h=4, w=5, out_p=p(out), opitch=15):
        return eng.lib.pano_fill_u8(eng.ctx(), img_p, i64(pitch), mask_p, i64(mpitch), h, w, 0, out_p,
                                    i64(opitch))
    assert call() == 0
    for bad in (dict(img_p=None), dict(mask_p=None), dict(out_p=None), dict(h=0), dict(w=0),
                dict(h=32769), dict(pitch=14), dict(mpitch=4), dict(opitch=14),
                dict(out_p=p(img), opitch=18)):
        assert call(**bad) == _lib.EINVAL, bad
        assert b"pano_fill_u8" in eng.lib.pano_last_error()
    sel = eng.lib.pano_select_u8
    assert sel(eng.ctx(), p(img), p(mask), p(out), p(out), i64(20)) == 0
    for bad in ((None, p(mask), p(out), p(out), 20), (p(img), None, p(out), p(out), 20),
                (p(img), p(mask), None, p(out), 20), (p(img), p(mask), p(out), None, 20),
                (p(img), p(mask), p(out), p(out), 0)):
        assert sel(eng.ctx(), *bad[:4], i64(bad[4])) == _lib.EINVAL, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------- the sphere
@pytest.mark.parametrize("name", ["open", "ring"])
def test_sphere_device(eng, name):
    geom, mosaic = view_cases.GEOMETRIES[name], view_cases.mosaic(name)
    width, rows = 64, 32
    sphere, sgeom = fill.sphere_device(mosaic, geom, width=width, eng=eng)
    assert sgeom == fill.sphere_geometry(width) and sgeom.closed
    assert tuple(sphere.shape) == (rows + 2, width, 3) == sgeom.shape + (3,)
    (image,), (mask,) = view.render_device(mosaic, geom, [view.equirect(width)], eng)
    image, mask, got = image.cpu().numpy(), mask.cpu().numpy(), sphere.cpu().numpy()
    assert 0 < mask.sum() < mask.size
    assert np.array_equal(got[1:-1][mask == 1], image[mask == 1])
    filled = fill.fill(image, mask, True, eng)
    assert np.array_equal(got[1:-1], filled)
    assert np.array_equal(got[0], np.roll(filled[0], width // 2, axis=0))
    assert np.array_equal(got[-1], np.roll(filled[-1], width // 2, axis=0))
    # its own view renders it back.  The forward steps from the rows 0 and `rows` go over a pole,
    # where theta turns by pi: their footprint is half the width and they come from a coarse level
    # (as the last row of view_model's sphere); the row beyond the far pole is the boundary row
    (back,), (back_mask,) = view.render_device(sphere, sgeom, [sgeom.own_view()], eng)
    assert back_mask[1:-1].all()
    assert np.array_equal(back.cpu().numpy()[1:rows], got[1:rows])
    # a valid mask: the mosaic is filled first
    valid = fm.blobs(*geom.shape, 6, 5.0, seed=2)
    with_valid, _ = fill.sphere_device(mosaic, geom, valid, width, eng)
    first = fill.fill(mosaic, valid, geom.closed, eng)
    assert np.array_equal(with_valid.cpu().numpy(),
                          fill.sphere_device(first, geom, None, width, eng)[0].cpu().numpy())
    # the default width: the mosaic's columns per turn
    assert fill.sphere_device(mosaic, geom, eng=eng)[1] == fill.sphere_geometry(fill.sphere_width(geom))


def _bright_mosaic():
    return fill_cases.noise(*view_cases.GEOMETRIES["open"].shape, 31, low=16)


def test_render_filled_device(eng):
    geom, mosaic = view_cases.GEOMETRIES["open"], _bright_mosaic()
    sphere, sgeom = fill.sphere_device(mosaic, geom, width=128, eng=eng)
    assert int(sphere.min()) >= 16                      # convex combinations of values >= 16
    background = (view.mip_device(sphere, eng), sgeom)
    # six faces, the whole sphere, and two looks whose centre pixel is a pole itself
    poles = [view.perspective(0.0, s * np.pi / 2, 0.0, 1.0, (5, 5)) for s in (1, -1)]
    views = view.cube_faces(64) + [view.equirect(64)] + poles
    mips = view.mip_device(mosaic, eng)
    images, masks = fill.render_filled_device(mips, geom, views, background, eng)
    plain, plain_masks = view.render_device(mips, geom, views, eng)
    behind, behind_masks = view.render_device(background[0], sgeom, views, eng)
    covered = 0
    for v, img, m, p, pm, b, bm in zip(views, images, masks, plain, plain_masks, behind, behind_masks):
        img, m, p, pm, b, bm = (t.cpu().numpy() for t in (img, m, p, pm, b, bm))
        assert img.shape == (v.h, v.w, 3) and np.array_equal(m, pm)
        assert np.array_equal(img[m == 1], p[m == 1])
        assert np.array_equal(img[m == 0], b[m == 0])
        assert bm.all() and img.min() >= 15
        covered += int(m.sum())
    assert 0 < covered < sum(v.w * v.h for v in views)
    for m in behind_masks[-2:]:                         # the pixels at the two poles
        assert int(m[2, 2]) == 1
    # a mosaic instead of its chain, an image instead of the background's chain: the same
    again, _ = fill.render_filled_device(mosaic, geom, views[:6], (sphere, sgeom), eng)
    for a, b in zip(again, images):
        assert torch.equal(a, b)


def test_multires_tiles_with_a_background(eng):
    geom, mosaic = view_cases.GEOMETRIES["open"], _bright_mosaic()
    mips = view.mip_device(mosaic, eng)
    sphere, sgeom = fill.sphere_device(mosaic, geom, width=128, eng=eng)
    names, crops = tiles.multires_tiles(mips, geom, 64, 16, eng, background=(sphere, sgeom))
    rows = tiles.multires_files(64, 16)
    assert names == [r[0] for r in rows] and len(crops) == len(rows)
    assert all(int(t.min()) >= 15 for t in crops)       # no black pixel anywhere
    # without a background: what it returned before, the plain faces with their black
    names, crops = tiles.multires_tiles(mips, geom, 64, 16, eng)
    faces = {l: view.render_device(mips, geom, view.cube_faces(16 << (l - 1)), eng)[0] for l in (1, 2, 3)}
    assert names == [r[0] for r in rows]
    for (_, l, face, y0, x0, th, tw), crop in zip(rows, crops):
        assert torch.equal(crop, faces[l][face][y0:y0 + th, x0:x0 + tw])
    assert any(int(t.max()) == 0 for t in crops)


# ----------------------------------------------------------------- command line
def test_cli_fill(eng, tmp_path, monkeypatch):
    import pickle
    import bundle_adj
    import stitcher as top
    from PIL import Image
    from pano360_amd import synth
    imgs, rots, intrs = synth.make_scene(5, 200, 120, sweep_deg=80.0, jitter=0.01, seed=9, kind="B")
    with open(tmp_path / "ba_RIG_s2.pkl", "wb") as fid:
        pickle.dump([bundle_adj.Image(im, r, k) for im, r, k in zip(imgs, rots, intrs)], fid,
                    protocol=pickle.HIGHEST_PROTOCOL)
    monkeypatch.chdir(tmp_path)

    def regions():
        with open(tmp_path / "ba_RIG_s2.pkl", "rb") as fid:
            return pickle.load(fid)
    plain = top.main([str(tmp_path / "RIG"), "-b", "linear", "-o", "plain.png", "--equirect", "64"])
    got = top.main([str(tmp_path / "RIG"), "-b", "linear", "-o", "m.png", "--fill", "--equirect", "64",
                    "--multires", "32", "--tile", "16", "--deepzoom"])
    mosaic, rect, geom, valid = top._stitch_device_valid(regions(), top.linear_blend, False, False)
    assert rect is None and np.array_equal(mosaic.cpu().numpy(), plain)
    valid = valid.cpu().numpy()
    assert 0 < valid.sum() < valid.size
    want = fill.fill(plain, valid, geom.closed, eng)
    assert np.array_equal(got, want) and np.array_equal(got[valid != 0], plain[valid != 0])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "m.png"))[..., ::-1], want)
    sphere, sgeom = fill.sphere_device(want, geom, eng=eng)
    (eq,), _ = fill.render_filled_device(want, geom, [view.equirect(64)], (sphere, sgeom), eng)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "m_equirect.png"))[..., ::-1], eq.cpu().numpy())
    # without --fill nothing changed: the equirect of the plain mosaic, black outside it
    (eq0,), _ = view.render_device(plain, geom, [view.equirect(64)], eng)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "plain_equirect.png"))[..., ::-1], eq0.cpu().numpy())
    assert (tmp_path / "m.dzi").exists() and (tmp_path / "m_multires" / "config.json").exists()
    # the existing function's results are what they were
    three = top._stitch_device_geometry(regions(), top.linear_blend, False, False)
    assert len(three) == 3 and three[1] is None and three[2] == geom
