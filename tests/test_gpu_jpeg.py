"""Device JPEG decode (pano_jpeg_decode through pano360_amd.jpeg): bit-exact with Pillow on the
host test matrix and on full-size frames, the Huffman stage against the NumPy model, batches,
determinism, the routing of read_images and the ingest / CLI paths."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import jpeg_model as M
from test_jpeg_host import MATRIX, make, pillow

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(t):
    return t.cpu().numpy()


def test_matrix_equals_pillow_in_one_batch(eng):
    from pano360_amd import jpeg as J
    frames = J.decode_device([b for _, b in MATRIX], eng)
    bad = [name for (name, blob), f in zip(MATRIX, frames)
           if not np.array_equal(_host(f), pillow(blob))]
    assert not bad, bad


def test_each_image_alone_equals_the_mixed_batch(eng):
    from pano360_amd import jpeg as J
    pick = MATRIX[::7]
    batch = J.decode_device([b for _, b in pick], eng)
    for (name, blob), f in zip(pick, batch):
        alone = J.decode_device([blob], eng)[0]
        assert np.array_equal(_host(alone), _host(f)), name


def _full(w, h, q, samp, rst, kind, seed):
    from pano360_amd import synth
    img = synth.make_frame(seed, w, h, kind)
    kw = {"quality": q, "subsampling": samp}
    if rst == "rows":
        kw["restart_marker_rows"] = 1
    elif rst:
        kw["restart_marker_blocks"] = rst
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


FULL = [(1920, 1080, 75, 2, None, "B"), (1920, 1080, 90, 1, "rows", "B"),
        (1920, 1080, 100, 0, 7, "A"), (3840, 2160, 90, 2, None, "B"),
        (3840, 2160, 95, 0, None, "B"), (3840, 2160, 95, 0, 4, "B"),
        (3840, 2160, 85, 2, "rows", "A")]


@pytest.mark.parametrize("case", FULL, ids=lambda c: "x".join(map(str, c[:2])) +
                         f"-q{c[2]}-s{c[3]}-rst{c[4]}-{c[5]}")
def test_full_size_equals_pillow(eng, case):
    from pano360_amd import jpeg as J
    blob = _full(*case, seed=11)
    got = _host(J.decode_device([blob], eng)[0])
    want = pillow(blob)
    assert got.shape == want.shape
    diff = np.argwhere(got != want)
    assert diff.size == 0, f"{len(diff)} values differ, first at {diff[:3].tolist()}"


def test_huffman_coefficients_equal_the_model(eng):
    from pano360_amd import jpeg as J
    pick = [(n, b) for n, b in MATRIX if not n.startswith("orient")][::3]
    _, coefs = J.decode_device([b for _, b in pick], eng, want_coefs=True)
    for (name, blob), c in zip(pick, coefs):
        hdr = J.parse(blob)
        want = M.coefficients(hdr, blob)
        assert np.array_equal(_host(c).astype(np.int32), want), name


def test_two_runs_are_bit_identical(eng):
    from pano360_amd import jpeg as J
    blobs = [_full(1920, 1080, 95, 0, None, "B", 3), _full(640, 480, 80, 2, 2, "A", 4),
             make(33, 17, subsampling=1)]
    a = [_host(f).copy() for f in J.decode_device(blobs, eng)]
    b = [_host(f) for f in J.decode_device(blobs, eng)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_read_images_routes_non_baseline_files_to_pillow(eng, tmp_path):
    from pano360_amd import jpeg as J
    img = np.random.default_rng(1).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    Image.fromarray(img).save(tmp_path / "base.jpg", quality=90)
    Image.fromarray(img).save(tmp_path / "prog.jpg", quality=90, progressive=True)
    Image.fromarray(img).save(tmp_path / "lossless.png")
    paths = [str(tmp_path / f) for f in ("base.jpg", "prog.jpg", "lossless.png")]
    frames, route = J.read_images(paths, eng)
    assert route == ["device", "pillow", "pillow"]
    for p, f in zip(paths, frames):
        with open(p, "rb") as fid:
            assert np.array_equal(_host(f), pillow(fid.read()))


def test_read_images_splits_large_sets_into_batches(eng, tmp_path):
    from pano360_amd import jpeg as J
    paths = []
    for k in range(7):
        p = tmp_path / f"f{k}.jpg"
        with open(p, "wb") as fid:
            fid.write(make(96 + 16 * k, 64 + 5 * k, seed=k, noise=True, subsampling=k % 3,
                           quality=90))
        paths.append(str(p))
    blobs = [open(p, "rb").read() for p in paths]
    headers = [J.parse(b) for b in blobs]
    budget = 3 * max(J.pack([h], [b])[2] for h, b in zip(headers, blobs))
    lens = [h.data_end - h.data_start for h in headers]
    big = lens.index(max(lens))
    batches, rejected = J.plan_batches(headers, budget, max_data=max(lens) - 1)
    assert len(batches) >= 2 and rejected == [big]
    frames, route = J.read_images(paths, eng, max_packed=budget, max_data=max(lens) - 1)
    assert route == ["pillow" if i == big else "device" for i in range(len(paths))]
    for b, f in zip(blobs, frames):
        assert np.array_equal(_host(f), pillow(b))


def _jpeg_dir(tmp_path):
    from pano360_amd import synth
    d = tmp_path / "imgs"
    d.mkdir()
    for k, (w, h) in enumerate([(160, 96), (161, 97), (320, 200)]):
        Image.fromarray(synth.make_frame(k, w, h, "B")).save(d / f"f{k}.jpg", quality=90)
    with open(d / "rot.jpg", "wb") as fid:
        fid.write(make(120, 64, orientation=6, subsampling=2, quality=92))
    Image.fromarray(synth.make_frame(9, 64, 48, "B")).save(d / "p.png")
    return str(d)


@pytest.mark.parametrize("shrink", [1, 2])
def test_ingest_device_equals_host(eng, tmp_path, shrink):
    from pano360_amd import stitcher
    d = _jpeg_dir(tmp_path)
    dev = stitcher.ingest(d, shrink)
    host = stitcher.ingest(d, shrink, decode="host")
    assert len(dev) == len(host) == 5
    for a, b in zip(dev, host):
        assert np.array_equal(_host(a), _host(b))
    assert any(_host(f).shape[:2] == (120 // shrink, 64 // shrink) for f in dev)


def test_cli_register_on_jpegs_equals_the_pillow_path(tmp_path):
    import torch
    from pano360_amd import synth
    pano = synth.make_frame(7, 4096, 2048, "B")
    rots, intrs = synth.make_cameras(4, 640, 360, step_deg=30.0, jitter=0.01, seed=3)
    frames = synth.render_rig(pano, rots, intrs, 640, 360, torch.device("cuda"))
    outs = []
    for decode in ("device", "host"):
        run = tmp_path / decode
        src = run / "rig"
        src.mkdir(parents=True)
        for k, f in enumerate(frames):
            Image.fromarray(f.cpu().numpy()[..., ::-1]).save(src / f"f{k}.jpg", quality=92)
        code = ("import sys, functools, numpy as np; sys.path.insert(0, %r); import stitcher; "
                "stitcher.ingest = functools.partial(stitcher.ingest, decode=%r); "
                "m = stitcher.main([%r, '-s', '1', '-b', 'linear', '--register']); "
                "np.save(sys.argv[1], m)" % (ROOT, decode, str(src)))
        out = run / "mosaic.npy"
        subprocess.run([sys.executable, "-c", code, str(out)], cwd=run, check=True, timeout=300)
        outs.append(np.load(out))
    assert outs[0].size > 0 and np.array_equal(outs[0], outs[1])
