"""GPU: the tile writers of pano360_amd/tiles.py.  The set of files is exactly what the host
functions name, and every tile is the bytes Pillow writes for the same crop of the level (Deep
Zoom: a level of view.mip_device; cube: view.render_device of view.cube_faces) downloaded."""
import json
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import view_cases
from test_jpeg_encode_host import pillow
from pano360_amd import tiles, view

pytestmark = pytest.mark.gpu


def _files_under(root):
    return {os.path.relpath(os.path.join(d, f), root).replace(os.sep, "/")
            for d, _, names in os.walk(root) for f in names}


def _read(path):
    with open(path, "rb") as fid:
        return fid.read()


def test_write_deepzoom(eng, tmp_path):
    from pano360_amd import synth
    mosaic = np.ascontiguousarray(synth.make_frame(3, 83, 37, "B"))
    assert mosaic.shape == (37, 83, 3)
    written = tiles.write_deepzoom(str(tmp_path / "out" / "m"), mosaic, tile=16, eng=eng)
    rows = tiles.deepzoom_files(37, 83, 16)
    assert _files_under(tmp_path / "out") == {"m.dzi"} | {"m_files/" + r[0] for r in rows}
    assert len(written) == 1 + len(rows) and all(os.path.isfile(p) for p in written)
    size = ET.fromstring(_read(tmp_path / "out" / "m.dzi"))[0]
    assert size.attrib == {"Height": "37", "Width": "83"}
    mips = view.mip_device(mosaic, eng)
    levels = [mips.level(l).cpu().numpy() for l in range(mips.n_levels)]
    assert np.array_equal(levels[0], mosaic)
    for name, l, y0, x0, th, tw in rows:
        want = pillow(levels[l][y0:y0 + th, x0:x0 + tw, ::-1])
        assert _read(tmp_path / "out" / "m_files" / name) == want, name
    # a chain built before serves as well, and the tile need not divide anything
    again = tiles.write_deepzoom(str(tmp_path / "again"), mips, tile=7, eng=eng)
    assert len(again) == 1 + len(tiles.deepzoom_files(37, 83, 7))
    assert _read(tmp_path / "again_files" / "0" / "0_0.jpg") == _read(tmp_path / "out" / "m_files" / "0" / "0_0.jpg")


def test_write_multires(eng, tmp_path):
    geom = view_cases.GEOMETRIES["open"]
    mosaic = view_cases.mosaic("open")
    out = tmp_path / "cube"
    written = tiles.write_multires(str(out), mosaic, geom, side=64, tile=16, eng=eng)
    rows = tiles.multires_files(64, 16)
    assert _files_under(out) == {"config.json"} | {r[0] for r in rows}
    assert len(written) == 1 + len(rows)
    config = json.loads(_read(out / "config.json"))
    assert config["type"] == "multires" and config["multiRes"]["maxLevel"] == 3 \
        and config["multiRes"]["cubeResolution"] == 64 and config["multiRes"]["tileResolution"] == 16
    mips = view.mip_device(mosaic, eng)
    covered = 0
    for l in (1, 2, 3):
        images, masks = view.render_device(mips, geom, view.cube_faces(16 << (l - 1)), eng)
        faces = [t.cpu().numpy() for t in images]
        covered += sum(int(m.any()) for m in masks)
        for name, level, face, y0, x0, th, tw in rows:
            if level == l:
                want = pillow(faces[face][y0:y0 + th, x0:x0 + tw, ::-1])
                assert _read(out / name) == want, name
    assert 0 < covered < 18                             # an open mosaic: some faces are black
    for s in "frblud":
        assert _read(out / "fallback" / f"{s}.jpg") == _read(out / "1" / f"{s}0_0.jpg")
    with pytest.raises(ValueError):
        tiles.write_multires(str(tmp_path / "none"), mosaic, geom, side=15, tile=16, eng=eng)
    assert not (tmp_path / "none").exists()


@pytest.mark.parametrize("crop", [False, True])
def test_cli_writes_both_pyramids(eng, tmp_path, monkeypatch, crop):
    import pickle
    import bundle_adj
    import stitcher as top
    from pano360_amd import synth
    imgs, rots, intrs = synth.make_scene(5, 200, 120, sweep_deg=80.0, jitter=0.01, seed=9, kind="B")
    regions = [bundle_adj.Image(im, r, k) for im, r, k in zip(imgs, rots, intrs)]
    with open(tmp_path / "ba_RIG_s2.pkl", "wb") as fid:
        pickle.dump(regions, fid, protocol=pickle.HIGHEST_PROTOCOL)
    monkeypatch.chdir(tmp_path)
    chains = []
    real = view.mip_device
    monkeypatch.setattr(view, "mip_device", lambda *a, **k: chains.append(1) or real(*a, **k))
    got = top.main([str(tmp_path / "RIG"), "-b", "linear", "-o", "m.jpg", "--deepzoom",
                    "--multires", "64", "--tile", "16"] + (["-c"] if crop else []))
    assert chains == [1]                                # one mip chain for both
    h, w = got.shape[:2]
    size = ET.fromstring(_read(tmp_path / "m.dzi"))[0]
    assert size.attrib == {"Height": str(h), "Width": str(w)}
    assert _files_under(tmp_path / "m_files") == {r[0] for r in tiles.deepzoom_files(h, w, 16)}
    assert _files_under(tmp_path / "m_multires") == \
        {"config.json"} | {r[0] for r in tiles.multires_files(64, 16)}
    top_level = len(tiles.deepzoom_levels(h, w)) - 1
    assert _read(tmp_path / "m_files" / str(top_level) / "0_0.jpg") == pillow(got[:16, :16, ::-1])
    with pytest.raises(SystemExit):
        top.parse_args([str(tmp_path / "RIG"), "--deepzoom"])
