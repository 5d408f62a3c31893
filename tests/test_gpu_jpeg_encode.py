"""The device JPEG encode (``jpeg.encode_device``, csrc/jpeg_enc.hip) against Pillow: the same
bytes over the host matrix, at full size, past 2^31 stream bits and from a strided crop view; its
quantised blocks against the NumPy model and the device decoder; run-to-run identity; and the
CLI's ``-o mosaic.jpg`` through the device path."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_encode_model as M
from test_jpeg_encode_host import KINDS, QUALITIES, RESIDUES, SMALL, SUBSAMPLINGS, content, pillow

pytestmark = pytest.mark.gpu


def _bgr(rgb):
    return np.ascontiguousarray(rgb[..., ::-1])


@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_matrix_equals_pillow(eng, subsampling):
    from pano360_amd import jpeg as J
    for quality in QUALITIES:
        for w, h in SMALL + RESIDUES[::3]:
            for kind in KINDS:
                rgb = content(kind, w, h)
                want = pillow(rgb, quality, subsampling)
                assert J.encode_device(rgb, quality, subsampling, "rgb", eng) == want, \
                    (w, h, kind, quality)
                assert J.encode_device(_bgr(rgb), quality, subsampling, "bgr", eng) == want


@pytest.mark.parametrize("quality", (1, 50, 100))
def test_every_residue_pair_420_equals_pillow(eng, quality):
    from pano360_amd import jpeg as J
    for w in range(17, 33):
        for h in range(17, 33):
            rgb = content("noise", w, h)
            assert J.encode_device(rgb, quality, 2, "rgb", eng) == pillow(rgb, quality, 2), (w, h)


@pytest.mark.parametrize("w,h,quality,subsampling", [
    (1920, 1080, 75, -1), (1920, 1080, 95, 0), (1920, 1080, 90, 1),
    (3840, 2160, 75, -1), (3840, 2160, 100, 0), (3840, 2160, 50, 1), (3841, 2161, 90, 2),
    (40000, 1200, 75, -1)])
def test_full_size_equals_pillow(eng, w, h, quality, subsampling):
    from pano360_amd import jpeg as J
    from pano360_amd import synth
    frame = synth.make_frame(w * 7 + h, w, h, "B")
    want = pillow(frame[..., ::-1], quality, subsampling)
    assert J.encode_device(frame, quality, subsampling, "bgr", eng) == want


def test_stream_past_2_31_bits_equals_pillow(eng):
    """12000 x 9000 noise at quality 100, 4:4:4: the entropy-coded segment passes 2^31 bits."""
    import torch
    from pano360_amd import jpeg as J
    gen = torch.Generator(device="cpu").manual_seed(11)
    rgb = torch.randint(0, 256, (9000, 12000, 3), generator=gen, dtype=torch.uint8).numpy()
    want = pillow(rgb, 100, 0)
    hdr = J.parse(want)
    assert (hdr.data_end - hdr.data_start) * 8 > 2 ** 31
    got = J.encode_device(rgb, 100, 0, "rgb", eng)
    assert len(got) == len(want) and got == want


def test_strided_crop_view_equals_pillow_of_the_copy(eng):
    import torch
    from pano360_amd import jpeg as J
    from pano360_amd import synth
    mosaic = torch.from_numpy(synth.make_frame(5, 1003, 517, "B")).to(eng.device)
    view = mosaic[37:480, 101:950]
    assert not view.is_contiguous()
    want = pillow(view.cpu().numpy()[..., ::-1], 75, -1)
    assert J.encode_device(view, eng=eng) == want


@pytest.mark.parametrize("subsampling", SUBSAMPLINGS)
def test_coefficients_equal_the_model_and_the_decoder(eng, subsampling):
    from pano360_amd import jpeg as J
    for w, h in ((8, 8), (23, 29), (130, 67)):
        rgb = content("frame", w, h)
        data, coefs = J.encode_device(rgb, 90, subsampling, "rgb", eng, want_coefs=True)
        want = M.quantized_blocks(rgb, 90, subsampling)
        assert np.array_equal(coefs.cpu().numpy(), want.astype(np.int16))
        # the device decoder of Pillow's bytes returns the same blocks: its DC prediction
        # undoes the encoder's differences, so the DC is absolute on both sides
        _, dec = J.decode_device([pillow(rgb, 90, subsampling)], eng, want_coefs=True)
        assert np.array_equal(dec[0].cpu().numpy(), coefs.cpu().numpy())


def test_two_runs_give_identical_bytes(eng):
    from pano360_amd import jpeg as J
    from pano360_amd import synth
    frame = synth.make_frame(3, 2000, 1500, "B")
    a = J.encode_device(frame, 90, -1, "bgr", eng)
    b = J.encode_device(frame, 90, -1, "bgr", eng)
    assert a == b


def test_growth_then_reuse_on_one_fresh_engine(eng):
    """The stream buffers are the context's and only grow: after a large image the small one is
    emitted (ORed) into a buffer longer than its stream that held the large one's bits."""
    from pano360_amd import engine
    from pano360_amd import jpeg as J
    fresh = engine.Engine(eng.device)
    small, large = content("frame", 16, 16), content("noise", 640, 480)
    first = J.encode_device(small, 75, -1, "rgb", fresh)
    assert first == pillow(small, 75, -1)
    assert J.encode_device(large, 95, -1, "rgb", fresh) == pillow(large, 95, -1)
    again = J.encode_device(small, 75, -1, "rgb", fresh)
    assert again == pillow(small, 75, -1) and again == first


def test_scan_tile_borders_equal_pillow(eng):
    """A scan workgroup takes 4096 values.  At 4:2:2, 512 x 256 is exactly 4096 blocks (one full
    tile) and 656 x 200 is 4100 (a second tile of four); 1024 x 512 noise at quality 95 has a
    stuffed stream of more than 2 x 4096 chunks of 64 bytes, so the stuffing scan crosses a tile
    as well."""
    from pano360_amd import jpeg as J
    for w, h, blocks in ((512, 256, 4096), (656, 200, 4100)):
        mcus = -(-w // 16) * -(-h // 8)
        assert 4 * mcus == blocks
        rgb = content("noise", w, h)
        assert J.encode_device(rgb, 75, 1, "rgb", eng) == pillow(rgb, 75, 1), (w, h)
    rgb = content("noise", 1024, 512)
    want = pillow(rgb, 95, -1)
    hdr = J.parse(want)
    assert hdr.data_end - hdr.data_start > 2 * 4096 * 64
    assert J.encode_device(rgb, 95, -1, "rgb", eng) == want


def test_write_routes_out_of_scope_to_pillow(eng, tmp_path):
    from pano360_amd import jpeg as J
    rgb = content("frame", 40, 30)
    assert J.write(str(tmp_path / "a.jpg"), rgb, order="rgb", eng=eng) == "device"
    assert (tmp_path / "a.jpg").read_bytes() == pillow(rgb)
    assert J.write(str(tmp_path / "b.jpg"), rgb,
                   quality=101, order="rgb", eng=eng) == "pillow"
    assert not J.encodable(rgb.astype(np.float32)) and not J.encodable(rgb, quality=0)
    with pytest.raises(ValueError):
        J.encode_device(rgb, quality=0, eng=eng)


@pytest.mark.parametrize("crop", [False, True])
def test_cli_jpeg_output_is_pillows_bytes_from_the_device(tmp_path, monkeypatch, crop):
    import torch
    from PIL import JpegImagePlugin  # noqa: F401  (registers the JPEG saver)
    from pano360_amd import stitcher, synth
    pano = synth.make_frame(7, 4096, 2048, "B")
    rots, intrs = synth.make_cameras(4, 640, 360, step_deg=30.0, jitter=0.01, seed=3)
    frames = synth.render_rig(pano, rots, intrs, 640, 360, torch.device("cuda"))
    src = tmp_path / "rig"
    src.mkdir()
    for k, f in enumerate(frames):
        Image.fromarray(f.cpu().numpy()[..., ::-1]).save(src / f"f{k}.jpg", quality=92)
    monkeypatch.chdir(tmp_path)
    real_save = Image.SAVE["JPEG"]

    def refuse(*args, **kwargs):
        raise AssertionError("the mosaic went through Pillow's JPEG encoder")

    monkeypatch.setitem(Image.SAVE, "JPEG", refuse)
    argv = [str(src), "-s", "1", "-b", "linear", "--register", "-o", "mosaic.jpg"]
    got = stitcher.main(argv + (["-c"] if crop else []))
    monkeypatch.setitem(Image.SAVE, "JPEG", real_save)
    assert got.size > 0
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(got[..., ::-1])).save(buf, "JPEG")
    assert (tmp_path / "mosaic.jpg").read_bytes() == buf.getvalue()
