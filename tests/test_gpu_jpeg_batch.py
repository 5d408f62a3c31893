"""GPU: the batched JPEG encode (pano_jpeg_encode_batch, jpeg.encode_batch_device).  Every file
of a batch must be the bytes Pillow writes for that image alone, whatever shares the call with it:
the cases put image boundaries inside the block kernel's workgroups (32 blocks), inside the
wave-per-block kernels' workgroups (4 blocks), and several whole streams inside one stuffing chunk's
neighbourhood."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_jpeg_encode_host import SUBSAMPLINGS, content, pillow

pytestmark = pytest.mark.gpu

MIXED = [(1, 1), (8, 8), (17, 33), (16, 16), (200, 1), (23, 29), (130, 67), (1, 200)]     # (w, h)


@functools.lru_cache(maxsize=None)
def _rgb(w, h):
    rgb = content("noise", w, h)
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(maxsize=None)
def _want(w, h, quality, subsampling):
    return pillow(_rgb(w, h), quality, subsampling)


def _mixed(eng, sizes, quality, subsampling, order, **kw):
    from pano360_amd import jpeg as J
    images = [np.array(_rgb(w, h) if order == "rgb" else _rgb(w, h)[..., ::-1]) for w, h in sizes]
    return J.encode_batch_device(images, quality, subsampling, order, eng, **kw)


def test_a_batch_of_one_equals_pillow(eng):
    from pano360_amd import jpeg as J
    rgb = content("frame", 130, 67)
    assert J.encode_batch_device([rgb], 90, -1, "rgb", eng) == [pillow(rgb, 90, -1)]
    assert J.encode_batch_device([rgb], 90, -1, "rgb", eng) == [J.encode_device(rgb, 90, -1, "rgb", eng)]


@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_mixed_sizes_in_one_call_equal_pillow(eng, subsampling):
    from pano360_amd import jpeg as J
    assert J.encode_blocks(1, 1, -1) == 6               # a 1 x 1 image at 4:2:0 is 6 blocks
    for quality in (1, 75, 100):
        for sizes in (MIXED, MIXED[::-1]):
            want = [_want(w, h, quality, subsampling) for w, h in sizes]
            for order in ("rgb", "bgr"):
                got = _mixed(eng, sizes, quality, subsampling, order)
                for size, a, b in zip(sizes, got, want):
                    assert a == b, (size, quality, order, sizes is MIXED)


def test_many_identical_images_give_identical_files(eng):
    """A DC predictor carried across images, a shifted offset or a shared final byte would make
    a later copy differ from the first; the white 1 x 1 streams are a few bytes each."""
    from pano360_amd import jpeg as J
    for rgb, copies in ((content("noise", 17, 33), 70), (content("white", 1, 1), 100)):
        for subsampling in (-1, 0):
            got = J.encode_batch_device([rgb] * copies, 75, subsampling, "rgb", eng)
            assert len(got) == copies and got[0] == pillow(rgb, 75, subsampling)
            assert all(g == got[0] for g in got)


def test_dense_0xff_streams_equal_pillow(eng):
    """Noise at quality 100, 4:4:4: the streams are dense in 0xFF, also at their ends."""
    from pano360_amd import jpeg as J
    images = [content("noise", 24, 24, seed) for seed in range(40)]
    want = [pillow(rgb, 100, 0) for rgb in images]
    assert sum(w.count(b"\xff\x00") for w in want) > 40
    assert J.encode_batch_device(images, 100, 0, "rgb", eng) == want


def test_tiles_cut_as_views_past_one_scan_tile(eng):
    """The real use: strided crop views, not copies.  64 tiles of 64 x 64 out of a 512 x 512
    tensor are 64 * 96 = 6144 blocks at 4:2:0, more than one scan tile of 4096; then the right
    and bottom edge tiles of a 500 x 500 tensor (52 wide or high)."""
    from pano360_amd import jpeg as J
    from pano360_amd import synth, tiles
    for side in (512, 500):
        bgr = np.ascontiguousarray(synth.make_frame(side, side, side, "B"))
        dev = torch.from_numpy(bgr).to(eng.device)
        grid = tiles.tile_grid(side, side, 64)
        if side == 500:
            grid = [g for g in grid if g[4] < 64 or g[5] < 64]
            assert len(grid) == 15
        else:
            assert len(grid) == 64 and sum(J.encode_blocks(64, 64) for _ in grid) > 4096
        views = [dev[y0:y0 + th, x0:x0 + tw] for _, _, y0, x0, th, tw in grid]
        assert not any(v.is_contiguous() for v in views)
        got = J.encode_batch_device(views, 75, -1, "bgr", eng)
        for (_, _, y0, x0, th, tw), g in zip(grid, got):
            assert g == pillow(bgr[y0:y0 + th, x0:x0 + tw, ::-1], 75, -1), (side, y0, x0)


def test_splitting_into_native_calls_gives_the_same_files(eng, monkeypatch):
    from pano360_amd import jpeg as J
    sizes = MIXED + MIXED[::-1]
    blocks = [J.encode_blocks(h, w, -1) for w, h in sizes]
    native = eng.lib.pano_jpeg_encode_batch_work_bytes
    budget = int(native(C.c_int64(max(blocks) + 12), 3))
    batches = J.plan_encode_batches(blocks, budget)
    assert len(batches) >= 3 and [i for b in batches for i in b] == list(range(len(sizes)))
    calls = []
    real = eng.lib.pano_jpeg_encode_batch
    monkeypatch.setattr(eng, "lib", _Spy(eng.lib, "pano_jpeg_encode_batch",
                                         lambda *a: calls.append(a[2]) or real(*a)))
    got = _mixed(eng, sizes, 75, -1, "rgb", max_work=budget)
    assert calls == [len(b) for b in batches]
    assert got == [_want(w, h, 75, -1) for w, h in sizes]


class _Spy:
    def __init__(self, lib, name, fn):
        self._lib, self._name, self._fn = lib, name, fn

    def __getattr__(self, name):
        return self._fn if name == self._name else getattr(self._lib, name)


def test_errors_are_raised_before_anything_is_queued(eng):
    from pano360_amd import _lib
    from pano360_amd import jpeg as J
    assert J.encode_batch_device([], eng=eng) == []
    good = torch.zeros((8, 8, 3), dtype=torch.uint8, device=eng.device)
    for bad in (good.float(), good[..., :2], good[0]):
        with pytest.raises(ValueError):
            J.encode_batch_device([good, bad], eng=eng)
    with pytest.raises(ValueError):
        J.encode_batch_device([good], order="gbr", eng=eng)
    # the native call: an error status, and the context still works afterwards
    lib = eng.lib
    qt = np.ascontiguousarray(J.quant_tables(75).astype(np.uint8))
    work_bytes = int(lib.pano_jpeg_encode_batch_work_bytes(C.c_int64(6), 1))
    work = torch.empty(work_bytes, dtype=torch.uint8, device=eng.device)
    table = (_lib.JpegImage * 1)()
    table[0].img, table[0].pitch, table[0].h, table[0].w = good.data_ptr(), good.stride(0), 8, 8
    streams, offsets = C.c_void_p(), C.c_void_p()

    def call(images, n, sub=2, work_bytes=work_bytes):
        return lib.pano_jpeg_encode_batch(
            eng.ctx(), images, n, 0, sub, qt.ctypes.data_as(C.c_void_p), C.c_void_p(work.data_ptr()),
            C.c_int64(work_bytes), C.byref(streams), C.byref(offsets))

    assert call(table, 0) == _lib.EINVAL
    assert call(None, 1) == _lib.EINVAL
    assert call(table, _lib.JPEG_BATCH_MAX + 1) == _lib.EINVAL
    assert call(table, 1, sub=3) == _lib.EINVAL
    assert call(table, 1, work_bytes=work_bytes - 1) == _lib.EINVAL
    table[0].pitch = 23
    assert call(table, 1) == _lib.EINVAL
    table[0].pitch = good.stride(0)
    assert call(table, 1) == 0 and offsets.value and streams.value
    offs = (C.c_int64 * 2).from_address(offsets.value)
    assert offs[0] == 0 and 0 < offs[1] < 64


def test_two_runs_give_the_same_bytes(eng):
    a = _mixed(eng, MIXED, 75, -1, "bgr")
    b = _mixed(eng, MIXED, 75, -1, "bgr")
    assert a == b
