"""GPU: the view stage (pano_mip_u8, pano_view_render) against its float64 model
(tests/view_model.py) on the cases of tests/view_cases.py.

Against the model: the masks are equal and every covered pixel is within 1 level, outside the pixels
whose model fx or fy lies within 1e-3 px of a coverage boundary (at most 1 % of a case:
tests/test_view_host.py).  Why 1: a float32 angle error of a few 1e-7 rad over the 0.02 - 0.09
rad/px of these mosaics is about 1e-5 px, far below half a level even on noise, so only rounding
ties can move.  How many pixels differ is printed, not asserted.  The identity views must return
the mosaic exactly: a systematic bias would show there."""
import functools

import numpy as np
import pytest
import torch

import view_cases
import view_model as vm
from pano360_amd import view

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _levels(name):
    levels = vm.mip_levels(view_cases.mosaic(name))
    for lv in levels:
        lv.setflags(write=False)
    return tuple(levels)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """[(image, mask, near)] of a case's views by the model, computed once."""
    geom_name, views = view_cases.CASES[case]
    geom = view_cases.GEOMETRIES[geom_name]
    out = []
    for v in views:
        img, mask = vm.render(_levels(geom_name), geom, v)
        near = vm.near_boundary(v, geom)
        for a in (img, mask, near):
            a.setflags(write=False)
        out.append((img, mask, near))
    return out


@functools.lru_cache(maxsize=None)
def _mips(name):
    return view.mip_device(view_cases.mosaic(name))


def _render(case, eng):
    geom_name, views = view_cases.CASES[case]
    images, masks = view.render_device(_mips(geom_name), view_cases.GEOMETRIES[geom_name], views, eng)
    return [t.cpu().numpy() for t in images], [t.cpu().numpy() for t in masks]


def _compare(case, images, masks):
    differing = total = 0
    for k, ((want, want_mask, near), got, got_mask) in enumerate(zip(_reference(case), images, masks)):
        keep = ~near
        assert got.shape == want.shape and got_mask.shape == want_mask.shape
        assert set(np.unique(got_mask)) <= {0, 1}
        assert np.array_equal(got_mask[keep], want_mask[keep]), (case, k)
        assert not got[got_mask == 0].any(), (case, k)
        both = keep & (want_mask == 1)
        delta = np.abs(got[both].astype(int) - want[both].astype(int))
        differing += int((delta > 0).any(axis=-1).sum())
        total += int(both.sum())
        assert delta.max(initial=0) <= 1, (case, k, int(delta.max()))
    print(f"{case}: {differing} of {total} compared pixels differ from the model (by 1 level)")


# ------------------------------------------------------------------ mip chain
@pytest.mark.parametrize("shape", [(33, 67), (1, 2)])
def test_mip_levels_equal_the_model(eng, shape):
    img = view_cases.noise(shape, 21)
    mips = view.mip_device(img, eng)
    want = vm.mip_levels(img)
    assert mips.n_levels == len(want) and mips.shape == shape
    for l, lv in enumerate(want):
        assert np.array_equal(mips.level(l).cpu().numpy(), lv), l
    host = view.mip(img, eng)                       # the host wrapper
    assert len(host) == len(want) and all(np.array_equal(a, b) for a, b in zip(host, want))
    # a crop view of a wider image needs no copy and gives the crop's chain
    wide = view_cases.noise((shape[0] + 2, shape[1] + 3), 22)
    crop = torch.from_numpy(wide).to(eng.device)[1:1 + shape[0], 2:2 + shape[1]]
    assert crop.stride(0) == 3 * (shape[1] + 3)          # a view: rows further apart than they are long
    cropped = view.mip_device(crop, eng)
    for l, lv in enumerate(vm.mip_levels(wide[1:1 + shape[0], 2:2 + shape[1]])):
        assert np.array_equal(cropped.level(l).cpu().numpy(), lv), l


# ------------------------------------------------------- views against the model
@pytest.mark.parametrize("case", [c for c in sorted(view_cases.CASES)
                                  if c not in ("tall_identity", "tall_rolled")])
def test_views_equal_the_model(eng, case):
    images, masks = _render(case, eng)
    _compare(case, images, masks)


def test_open_mosaic_view_is_partly_outside(eng):
    _, masks = _render("open_partly_outside", eng)
    share = masks[0].mean()
    assert 0.2 < share < 0.8 and masks[0][:, 0].all() and not masks[0][:, -1].any()


# -------------------------------------------------------------------- identities
@pytest.mark.parametrize("case, shift", [("tall_identity", 0), ("tall_rolled", view_cases.ROLL)])
def test_own_view_returns_the_mosaic_exactly(eng, case, shift):
    (image,), (mask,) = _render(case, eng)
    want = np.roll(view_cases.mosaic("tall"), -shift, axis=1)
    # rows 0 and H - 1 sit on the coverage boundary (fy = 0, fy = H - 1): float32 decides whether
    # they are covered; every other pixel is, and every covered pixel is the mosaic's
    assert mask[1:-1].all()
    assert np.array_equal(image[mask == 1], want[mask == 1]) and not image[mask == 0].any()
    _compare(case, [image], [mask])


# ------------------------------------------------------------------- the batch
def test_a_batch_equals_its_views_rendered_alone(eng):
    geom, mips = view_cases.GEOMETRIES["ring"], _mips("ring")
    images, masks = view.render_device(mips, geom, view_cases.BATCH_VIEWS, eng)
    assert [tuple(t.shape) for t in images] == [(1, 1, 3), (3, 65, 3), (24, 40, 3)]
    assert [tuple(t.shape) for t in masks] == [(1, 1), (3, 65), (24, 40)]
    for v, image, mask in zip(view_cases.BATCH_VIEWS, images, masks):
        (alone,), (alone_mask,) = view.render_device(mips, geom, [v], eng)
        assert torch.equal(alone, image) and torch.equal(alone_mask, mask)
    # and in another order
    back, back_masks = view.render_device(mips, geom, view_cases.BATCH_VIEWS[::-1], eng)
    assert all(torch.equal(a, b) for a, b in zip(back[::-1], images))
    assert all(torch.equal(a, b) for a, b in zip(back_masks[::-1], masks))


def test_two_runs_give_the_same_bytes_and_inputs_are_not_written(eng):
    geom, views = view_cases.GEOMETRIES["sphere"], view_cases.CASES["sphere_cube"][1]
    mosaic = torch.from_numpy(view_cases.mosaic("sphere")).to(eng.device)
    before = mosaic.clone()
    mips = view.mip_device(mosaic, eng)
    chain = mips.buffer.clone()
    first = view.render_device(mips, geom, views, eng)
    second = view.render_device(mips, geom, views, eng)
    for a, b in zip(first[0] + first[1], second[0] + second[1]):
        assert torch.equal(a, b)
    assert torch.equal(mosaic, before) and torch.equal(mips.buffer, chain)
    again = view.mip_device(mosaic, eng)
    for l in range(mips.n_levels):
        assert torch.equal(again.level(l), mips.level(l))
    # a mosaic in place of its chain: the chain is built first, the result is the same
    direct = view.render_device(mosaic, geom, views, eng)
    assert all(torch.equal(a, b) for a, b in zip(direct[0] + direct[1], first[0] + first[1]))


def test_host_wrappers_equal_the_device_calls(eng):
    geom, views = view_cases.GEOMETRIES["open"], view_cases.CASES["open_partly_outside"][1]
    images, masks = view.render(view_cases.mosaic("open"), geom, views, eng)
    dev_images, dev_masks = _render("open_partly_outside", eng)
    assert isinstance(images[0], np.ndarray) and images[0].dtype == np.uint8 == masks[0].dtype
    assert np.array_equal(images[0], dev_images[0]) and np.array_equal(masks[0], dev_masks[0])


def test_native_call_refuses_what_it_cannot_render(eng):
    import ctypes as C
    from pano360_amd import _lib
    geom, mips = view_cases.GEOMETRIES["ring"], _mips("ring")
    table, record = view.view_records([view.equirect(8)], geom, geom.shape)
    offs = (C.c_int64 * len(mips.offsets))(*mips.offsets)
    # null outputs, a level count that is not the chain's, a mosaic that claims to close
    assert eng.lib.pano_view_render(eng.ctx(), _lib._ptr(mips.buffer), offs, mips.n_levels,
                                    C.byref(record), table, 1) == _lib.EINVAL
    out = torch.empty(8 * 4 * 4, dtype=torch.uint8, device=eng.device)
    table[0].image, table[0].mask = out.data_ptr(), out.data_ptr() + 96
    assert eng.lib.pano_view_render(eng.ctx(), _lib._ptr(mips.buffer), offs, mips.n_levels - 1,
                                    C.byref(record), table, 1) == _lib.EINVAL
    record.w = 60
    assert eng.lib.pano_view_render(eng.ctx(), _lib._ptr(mips.buffer), offs, mips.n_levels,
                                    C.byref(record), table, 1) == _lib.EINVAL


# ------------------------------------------------------------------------- the CLI
@pytest.mark.parametrize("crop", [False, True])
def test_cli_writes_the_views_beside_the_mosaic(eng, tmp_path, monkeypatch, crop):
    import pickle
    import bundle_adj
    import stitcher as top
    from PIL import Image
    from pano360_amd import synth
    imgs, rots, intrs = synth.make_scene(5, 200, 120, sweep_deg=80.0, jitter=0.01, seed=9, kind="B")
    regions = [bundle_adj.Image(im, r, k) for im, r, k in zip(imgs, rots, intrs)]
    with open(tmp_path / "ba_RIG_s2.pkl", "wb") as fid:
        pickle.dump(regions, fid, protocol=pickle.HIGHEST_PROTOCOL)
    monkeypatch.chdir(tmp_path)
    calls = []
    real = view.render_device

    def spy(mosaic, geom, views, eng=None):
        out = real(mosaic, geom, views, eng)
        calls.append((mosaic, geom, list(views), out))
        return out

    monkeypatch.setattr(view, "render_device", spy)
    got = top.main([str(tmp_path / "RIG"), "-b", "linear", "-o", "m.png", "--equirect", "64", "--cube", "16",
                    "--view", "0,0,60,48x32", "--view=-20,5,40,31x17"] + (["-c"] if crop else []))
    names = ["m_view0.png", "m_view1.png", "m_equirect.png"] + [f"m_cube_{f}.png" for f in view.CUBE_FACES]
    (mosaic, geom, views, (images, masks)), = calls                  # one batch
    assert geom.shape == got.shape[:2] and geom.is_crop == crop and len(views) == 9
    assert np.array_equal(mosaic.cpu().numpy(), got)
    assert [(v.w, v.h) for v in views] == [(48, 32), (31, 17), (64, 32)] + [(16, 16)] * 6
    assert masks[0].any() and masks[3].any() and not masks[5].any()     # front: seen; back: not
    for name, image in zip(names, images):
        assert np.array_equal(np.asarray(Image.open(tmp_path / name))[..., ::-1], image.cpu().numpy())
    # the look at the mosaic's centre against the model on the mosaic the run returned
    want, want_mask = vm.render(vm.mip_levels(got), geom, views[0])
    keep = ~vm.near_boundary(views[0], geom)
    assert np.array_equal(masks[0].cpu().numpy()[keep], want_mask[keep])
    delta = np.abs(images[0].cpu().numpy().astype(int) - want.astype(int))[keep & (want_mask == 1)]
    assert delta.max(initial=0) <= 1
