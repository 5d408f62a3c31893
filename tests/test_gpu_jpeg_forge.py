"""Device JPEG decode of the hand-forged streams of tests/test_jpeg_forge_host.py: each equals
Pillow bit for bit in one batch and alone, the Huffman coefficients equal the blocks that were
coded, two runs agree, the sync rounds equal ``jpeg_model.sync_rounds``, full-size streams
(4K with FF-dense tables and no RST, 4K with deep tables and DRI 1, 1080p per knob group, the
widest and tallest frames Pillow takes) decode, and ``read_images`` routes in-scope and
out-of-scope forgeries.  Only streams that passed the host checks (model equals Pillow, rounds
under the bound) are sent here."""
import ctypes as C

import numpy as np
import pytest

import jpeg_model as M
from pano360_amd import _lib
from pano360_amd import jpeg as J
from test_jpeg_forge_host import FULL, OUT_OF_SCOPE, ROUND_BOUND, full, on_device, sync_stress
from test_jpeg_host import pillow

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def feng():
    """An engine of this module's own: its timing switch leaves the session engine alone."""
    from pano360_amd import engine
    return engine.Engine()


def _host(t):
    return t.cpu().numpy()


def test_forged_streams_equal_pillow_in_one_batch(feng):
    streams = on_device()
    frames = J.decode_device([f.blob for _, f in streams], feng)
    bad = [n for (n, f), got in zip(streams, frames) if not np.array_equal(_host(got),
                                                                           pillow(f.blob))]
    assert not bad, bad


def test_each_forged_stream_alone_equals_pillow(feng):
    bad = []
    for n, f in on_device():
        if not np.array_equal(_host(J.decode_device([f.blob], feng)[0]), pillow(f.blob)):
            bad.append(n)
    assert not bad, bad


def test_huffman_coefficients_equal_the_coded_blocks(feng):
    streams = on_device()
    _, coefs = J.decode_device([f.blob for _, f in streams], feng, want_coefs=True)
    bad = [n for (n, f), c in zip(streams, coefs)
           if not np.array_equal(_host(c).astype(np.int32), f.blocks)]
    assert not bad, bad


def test_two_runs_are_bit_identical(feng):
    blobs = [f.blob for _, f in on_device()][::3]
    a = [_host(x).copy() for x in J.decode_device(blobs, feng)]
    b = [_host(x) for x in J.decode_device(blobs, feng)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _rounds(eng, blob):
    lib = eng.lib
    names = [lib.pano_kernel_name(k).decode() for k in range(lib.pano_kernel_count())]
    kid = names.index("jpeg_huff_sync_kernel")
    _lib.check(lib.pano_timing_enable(eng.ctx(), 1), "pano_timing_enable")
    try:
        J.decode_device([blob], eng)
        ms, cnt = C.c_double(0), C.c_int(0)
        _lib.check(lib.pano_timing_read(eng.ctx(), kid, C.byref(ms), C.byref(cnt)),
                   "pano_timing_read")
    finally:
        _lib.check(lib.pano_timing_enable(eng.ctx(), 0), "pano_timing_enable")
    return cnt.value - 1


def test_sync_rounds_equal_the_model(feng):
    streams = sync_stress()
    want = {n: M.sync_rounds(f.hdr, f.blob) for n, f in streams}
    assert all(r <= ROUND_BOUND for r in want.values())
    got = {n: _rounds(feng, f.blob) for n, f in streams}
    print("device sync rounds:", got)
    assert got == want
    assert max(got.values()) >= 3


@pytest.mark.parametrize("name", FULL)
def test_full_size_stream_equals_pillow(feng, name):
    f = full(name)
    got = _host(J.decode_device([f.blob], feng)[0])
    want = pillow(f.blob)
    assert got.shape == want.shape
    diff = np.argwhere(got != want)
    assert diff.size == 0, f"{len(diff)} values differ, first at {diff[:3].tolist()}"


def test_full_size_coefficients_equal_the_coded_blocks(feng):
    for name in ("uhd-ffdense", "uhd-deep-dri1"):
        f = full(name)
        _, coefs = J.decode_device([f.blob], feng, want_coefs=True)
        assert np.array_equal(_host(coefs[0]).astype(np.int32), f.blocks), name


def test_read_images_routes_forged_files(feng, tmp_path):
    files = [(n, f.blob, "device") for n, f in on_device()[::4]]
    for kind in ("440", "411", "xmp", "second-exif", "orientation-long"):
        files.append((kind, OUT_OF_SCOPE[kind](), "pillow"))
    files.insert(3, files.pop())
    paths = []
    for k, (n, blob, _) in enumerate(files):
        p = tmp_path / f"{k:03d}-{n}.jpg"
        p.write_bytes(blob)
        paths.append(str(p))
    frames, route = J.read_images(paths, feng)
    assert route == [r for _, _, r in files]
    for (n, blob, _), got in zip(files, frames):
        assert np.array_equal(_host(got), pillow(blob)), n
