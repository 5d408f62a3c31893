"""CPU: the NumPy restatement of the device PNG encoder (tests/png_model.py) is lossless - its
scanlines open in Pillow and un-filter by an independent routine - the run tokeniser stands for
its input, and the host side of ``pano360_amd.png`` (the container, ``encodable``) is right."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import png_model as M

KINDS = ("smooth", "noise", "flat", "gradient")
SHAPES = ((1, 1), (1, 7), (5, 1), (3, 2), (41, 97))     # (w, h)


def content(kind, w, h, seed=5):
    """uint8 RGB [h][w][3]."""
    from pano360_amd import synth
    if kind == "smooth":
        return np.ascontiguousarray(synth.make_frame(seed, max(w, 8), max(h, 8), "B")[:h, :w])
    if kind == "noise":
        return synth.make_frame(seed, w, h, "A")
    if kind == "flat":
        return np.broadcast_to(np.array([77, 130, 200], np.uint8), (h, w, 3)).copy()
    if kind == "gradient":
        y, x = np.mgrid[:h, :w]
        return np.stack([3 * x + y, 2 * y + 5, 255 - x - 2 * y], axis=2).astype(np.uint8)
    raise ValueError(kind)


def banded(w=256, h=192, seed=5):
    """A smooth frame whose top and bottom thirds are black (a cropped mosaic's bands)."""
    rgb = content("smooth", w, h, seed)
    rgb[:h // 3] = 0
    rgb[h - h // 3:] = 0
    return rgb


def unfilter(lines, w):
    """PNG un-filtering at 3 bytes per pixel, byte by byte as the specification words it."""
    h = lines.shape[0]
    out = np.zeros((h, 3 * w), np.uint8)
    for y in range(h):
        kind, row = int(lines[y, 0]), lines[y, 1:]
        assert 0 <= kind <= 4
        for i in range(3 * w):
            a = int(out[y, i - 3]) if i >= 3 else 0
            b = int(out[y - 1, i]) if y else 0
            c = int(out[y - 1, i - 3]) if y and i >= 3 else 0
            if kind == 0:
                pred = 0
            elif kind == 1:
                pred = a
            elif kind == 2:
                pred = b
            elif kind == 3:
                pred = (a + b) // 2
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
            out[y, i] = (int(row[i]) + pred) & 255
    return out.reshape(h, w, 3)


def chunks(data):
    """[(kind, body)] of a PNG file; every length and CRC checked."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(data):
        (length,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + length]
        assert len(body) == length
        (crc,) = struct.unpack(">I", data[at + 8 + length:at + 12 + length])
        assert crc == zlib.crc32(kind + body), kind
        out.append((kind, body))
        at += 12 + length
    assert at == len(data)
    return out


def check_structure(data, w, h):
    """The chunk sequence of ``png.container`` and its IHDR; returns the IDAT bodies."""
    cs = chunks(data)
    kinds = [k for k, _ in cs]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and cs[-1][1] == b""
    assert len(kinds) >= 3 and set(kinds[1:-1]) == {b"IDAT"}
    assert cs[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    return [b for k, b in cs if k == b"IDAT"]


@pytest.mark.parametrize("kind", KINDS)
def test_model_scanlines_are_lossless(kind):
    from pano360_amd import png
    for w, h in SHAPES:
        rgb = content(kind, w, h)
        lines = M.scanlines(rgb)
        assert lines.shape == (h, 1 + 3 * w) and lines[:, 0].max() <= 4
        data = png.container(zlib.compress(lines.tobytes()), w, h)
        back = Image.open(io.BytesIO(data))
        assert back.mode == "RGB" and back.size == (w, h)
        assert np.array_equal(np.asarray(back), rgb), (kind, w, h)
        assert np.array_equal(unfilter(lines, w), rgb), (kind, w, h)


def test_model_choice_is_the_first_minimum():
    flat = content("flat", 9, 4)
    lines = M.scanlines(flat)
    # row 0: Sub and Paeth leave only the first pixel, the smallest sum: Sub (1) comes first
    assert lines[0, 0] == 1
    # below: Up and Paeth are all zero: Up (2) comes first
    assert list(lines[1:, 0]) == [2, 2, 2] and not lines[1:, 1:].any()
    for k in range(5):
        forced = M.scanlines(content("noise", 13, 6), choice=k)
        assert np.array_equal(unfilter(forced, 13), content("noise", 13, 6))


def test_model_tokens_stand_for_the_data():
    rng = np.random.default_rng(3)
    C = 1024
    cases = [b"", b"a", b"ab", bytes(range(256)), bytes(4 * C),
             rng.integers(0, 256, 3 * C + 5, dtype=np.uint8).tobytes()]
    for run in (2, 3, 4, 258, 259, 260, 261, 262, 517):
        cases.append(b"ab" + b"c" * run + b"de")
    for start in range(C - 2, C + 3):
        cases.append(rng.integers(0, 256, start, dtype=np.uint8).tobytes() + b"\x07" * 300 + b"zz")
    for data in cases:
        toks = M.tokens(data, C)
        assert len(toks) == max(1, -(-len(data) // C))
        assert M.expand(data, toks) == data
        for c, chunk in enumerate(toks):
            for pos, length in chunk:
                assert c * C <= pos and pos + max(length, 1) <= min((c + 1) * C, len(data))
                assert length == 0 or (3 <= length <= 258 and pos >= 1)
    # a run is one literal and as few matches as its length allows
    assert M.tokens(b"ab" + b"c" * 517 + b"de", C)[0] == \
        [(0, 0), (1, 0), (2, 0), (3, 258), (261, 258), (519, 0), (520, 0)]
    assert M.tokens(b"c" * 4, C)[0] == [(0, 0), (1, 3)]
    assert M.tokens(b"c" * 3, C)[0] == [(0, 0), (1, 0), (2, 0)]
    # across a chunk border the run goes on without a literal
    assert M.tokens(b"c" * 12, 8) == [[(0, 0), (1, 7)], [(8, 4)]]


def test_container_chunks_and_header():
    from pano360_amd import png
    rgb = content("noise", 41, 97)
    z = zlib.compress(M.scanlines(rgb).tobytes())
    whole = png.container(z, 41, 97)
    assert check_structure(whole, 41, 97) == [z]
    cut = png.container(z, 41, 97, idat_bytes=100)
    parts = check_structure(cut, 41, 97)
    assert len(parts) == -(-len(z) // 100) > 1 and all(len(p) <= 100 for p in parts)
    assert b"".join(parts) == z
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(cut))), rgb)
    for bad in (0, 1 << 31):
        with pytest.raises(ValueError):
            png.container(z, 41, 97, idat_bytes=bad)
    with pytest.raises(ValueError):
        png.container(z, 0, 97)
    assert png.CHUNK == M.CHUNK == 65536


def test_encodable():
    from pano360_amd import png
    assert png.encodable(np.zeros((4, 5, 3), np.uint8))
    assert png.encodable(np.zeros((1, 1, 3), np.uint8))
    for channels in (1, 2, 4):
        assert not png.encodable(np.zeros((4, 5, channels), np.uint8))
    assert not png.encodable(np.zeros((4, 5), np.uint8))
    for dtype in (np.int8, np.uint16, np.float32):
        assert not png.encodable(np.zeros((4, 5, 3), dtype))
    assert not png.encodable(np.zeros((0, 5, 3), np.uint8))
    assert not png.encodable(np.zeros((4, 0, 3), np.uint8))
    with pytest.raises(ValueError):
        png.filter_device(np.zeros((4, 5, 4), np.uint8))
    with pytest.raises(ValueError):
        png.filter_device(np.zeros((4, 5, 3), np.uint8), order="rbg")
