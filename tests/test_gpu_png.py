"""The device PNG encode (``pano360_amd.png``, csrc/png_enc.hip): the filter stage against the
NumPy model byte for byte; the length-limited code builder against a package-merge written here;
the deflate coder against ``zlib.decompress`` on the edge cases of its run tokeniser, of its
chunking and past 2^31 stream bits; its size against zlib's ``Z_RLE``; whole files through
Pillow; and the CLI's ``-o mosaic.png`` through the device path."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import png_model as M
from test_png_host import KINDS, SHAPES, banded, check_structure, content

pytestmark = pytest.mark.gpu

FILTER_SHAPES = SHAPES + ((33, 65), (64, 97))
# pano_deflate_lengths is a package-merge: its cost IS the optimum.  Largest excess over the
# vectors below, measured on the MI355X: 0.000 % for every (n_sym, max_bits); the bound stays there.
LENGTHS_EXCESS = 0.0
# The coder against zlib Z_RLE on the same bytes, beyond zlib's own cost of cutting the input
# into independent 64 KiB pieces (recomputed per input below).  A Python restatement of the coder
# (same tokens, package-merge lengths, header) gives -0.238 % (smooth), +0.051 % (noise) and
# +0.109 % (banded, whose 64 KiB pieces are mostly runs: few symbols, so the block headers weigh
# most); rounded up to the next 0.5 %.  The device's own figures are printed below and go into
# DESIGN 5h.  The issue's cap is 3 %.
CODER_EXCESS = 0.005


def _bgr(rgb):
    return np.ascontiguousarray(rgb[..., ::-1])


# ---- the filter stage --------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_filter_equals_the_model(eng, order):
    from pano360_amd import png
    for w, h in FILTER_SHAPES:
        for kind in KINDS:
            rgb = content(kind, w, h)
            got = png.filter_device(rgb if order == "rgb" else _bgr(rgb), order, eng)
            assert tuple(got.shape) == (h, 1 + 3 * w)
            assert np.array_equal(got.cpu().numpy(), M.scanlines(rgb)), (w, h, kind)


def test_filter_of_a_pitched_crop_view(eng):
    import torch
    from pano360_amd import png
    big = content("smooth", 150, 120)
    dev = torch.from_numpy(_bgr(big)).to(eng.device)
    view = dev[7:104, 11:52]
    assert not view.is_contiguous() and tuple(view.shape) == (97, 41, 3)
    want = M.scanlines(big[7:104, 11:52])
    assert np.array_equal(png.filter_device(view, "bgr", eng).cpu().numpy(), want)
    assert np.array_equal(png.filter_device(dev.flip(2)[7:104, 11:52], "rgb", eng).cpu().numpy(), want)


# ---- the code lengths --------------------------------------------------------------------------
def package_merge(freq, max_bits):
    """Optimal length-limited code lengths (Larmore and Hirschberg), items as explicit lists of
    the leaves they hold."""
    used = sorted((int(f), i) for i, f in enumerate(freq) if f > 0)
    lens = np.zeros(len(freq), np.int64)
    if len(used) == 1:
        lens[used[0][1]] = 1
    if len(used) < 2:
        return lens
    leaves = [(f, (i,)) for f, i in used]
    level = list(leaves)
    for _ in range(max_bits - 1):
        packages = [(level[k][0] + level[k + 1][0], level[k][1] + level[k + 1][1])
                    for k in range(0, len(level) - 1, 2)]
        level = sorted(leaves + packages, key=lambda item: item[0])
    for _, held in level[:2 * len(used) - 2]:
        for i in held:
            lens[i] += 1
    return lens


def _fibonacci(k):
    a = [1, 1]
    while len(a) < k:
        a.append(a[-1] + a[-2])
    return a[:k]


def length_vectors(n_sym, max_bits):
    rng = np.random.default_rng(1000 * n_sym + max_bits)
    out = []
    for at in (0, n_sym // 2, n_sym - 1):
        v = np.zeros(n_sym, np.int64)
        v[at] = 1 + at
        out.append(("one", v))
    v = np.zeros(n_sym, np.int64)
    v[1], v[n_sym - 1] = 1000, 1
    out.append(("two", v))
    out.append(("equal", np.full(n_sym, 7, np.int64)))
    out.append(("equal-but-one", np.r_[np.full(n_sym - 1, 7), 1].astype(np.int64)))
    # 22 Fibonacci frequencies need depth 21 unrestricted, 9 already pass 7 bits
    for k in (2, 3, 8, 9, 10, 12, 15, 16, 17, 19, 22, 23, 30, 40, 44):
        if k <= n_sym:
            v = np.zeros(n_sym, np.int64)
            v[rng.permutation(n_sym)[:k]] = _fibonacci(k)
            out.append((f"fibonacci-{k}", v))
    for trial in range(12):
        k = int(rng.integers(2, n_sym + 1)) if trial % 3 else int(rng.integers(2, 12))
        v = np.zeros(n_sym, np.int64)
        v[rng.choice(n_sym, k, replace=False)] = rng.integers(1, 1 << int(rng.integers(1, 20)), k)
        out.append((f"sparse-{trial}", v))
    return out


@pytest.mark.parametrize("n_sym,max_bits", [(286, 15), (30, 15), (19, 7)])
def test_code_lengths_against_package_merge(eng, n_sym, max_bits):
    from pano360_amd import png
    worst = 0.0
    for name, freq in length_vectors(n_sym, max_bits):
        got = png.code_lengths_device(freq, max_bits, eng).astype(np.int64)
        used = int((freq > 0).sum())
        assert np.array_equal(got > 0, freq > 0), name
        assert got.max() <= max_bits, name
        if used == 1:
            assert got.sum() == 1, name
        else:
            assert sum(1 << (max_bits - int(v)) for v in got[got > 0]) == 1 << max_bits, name
        best = int((package_merge(freq, max_bits) * freq).sum())
        cost = int((got * freq).sum())
        excess = cost / best - 1
        worst = max(worst, excess)
        print(f"lengths ({n_sym}, {max_bits}) {name}: cost {cost}, optimum {best}, "
              f"excess {100 * excess:.4f} %")
        assert cost >= best, name                       # (else the reference is not the optimum)
        assert excess <= LENGTHS_EXCESS <= 0.03, name
    print(f"lengths ({n_sym}, {max_bits}): worst excess {100 * worst:.4f} %")


# ---- the deflate coder -------------------------------------------------------------------------
def _check_deflate(png, eng, x, what):
    z = png.deflate_device(x, eng)
    assert z[:2] == b"\x78\x01", what
    assert zlib.decompress(z) == x, what
    assert int.from_bytes(z[-4:], "big") == zlib.adler32(x), what
    assert png.deflate_device(x, eng) == z, what
    return z


def test_deflate_round_trips_the_edge_cases(eng):
    from pano360_amd import png
    C = png.CHUNK
    rng = np.random.default_rng(17)

    def noise(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    cases = {"empty": b"", "one": b"q", "two": b"qr", "two equal": b"qq",
             "every byte once": bytes(range(256)), "noise": noise(5000)}
    for run in (2, 3, 4, 258, 259, 260, 261, 262, 517):
        cases[f"run of {run}"] = b"ab" + b"c" * run + b"de"
        cases[f"run of {run} at the start"] = b"c" * run + b"de"
    for start in range(C - 2, C + 3):
        head = noise(start - 1) + b"\x01"
        cases[f"run from {start}"] = head + b"\x07" * 300 + b"zz"
        cases[f"short run from {start}"] = head + b"\x07" * 3 + b"\x08"
    for n in (C - 1, C, C + 1, 3 * C + 5):
        cases[f"{n} bytes of noise"] = noise(n)
        cases[f"{n} equal bytes"] = b"\x55" * n
    cases["4 chunks of zeros"] = bytes(4 * C)
    # values repeated 1, 1, 2, 3, ... times and shuffled: a skewed histogram of 22 symbols
    fib = np.repeat(np.arange(22, dtype=np.uint8), _fibonacci(22))
    assert len(fib) == 46367
    cases["fibonacci-skewed"] = rng.permutation(fib).tobytes()
    for what, x in cases.items():
        z = _check_deflate(png, eng, x, what)
        if what == "empty":
            assert zlib.decompressobj(-15).decompress(z[2:-4]) == b"" and len(z) < 40
        if what == "4 chunks of zeros":
            assert len(z) < 1000                    # runs, not literals, across the chunk borders


def test_deflate_growth_then_reuse_on_one_engine(eng):
    """The stream buffers are the context's and only grow: after 3 chunks + 5 bytes of noise the
    one byte is emitted (ORed) into a buffer that held the long stream's bits."""
    from pano360_amd import engine, png
    fresh = engine.Engine(eng.device)
    noise = np.random.default_rng(29).integers(0, 256, 3 * png.CHUNK + 5, dtype=np.uint8).tobytes()
    first = _check_deflate(png, fresh, b"q", "one byte")
    _check_deflate(png, fresh, noise, "noise")
    assert _check_deflate(png, fresh, b"q", "one byte again") == first


def test_deflate_past_2_31_stream_bits(eng):
    """280 MB of device-generated noise: the bit offsets pass 2^31 (the only large case)."""
    import torch
    from pano360_amd import png
    gen = torch.Generator(device=eng.device).manual_seed(23)
    data = torch.randint(0, 256, (280 * 1000 * 1000,), generator=gen, dtype=torch.uint8,
                         device=eng.device)
    z = png.deflate_device(data, eng)
    assert (len(z) - 6) * 8 > 2 ** 31
    x = data.cpu().numpy()
    back = zlib.decompress(z)
    assert len(back) == x.size and np.array_equal(np.frombuffer(back, np.uint8), x)
    assert int.from_bytes(z[-4:], "big") == zlib.adler32(x)
    assert png.deflate_device(data, eng) == z


def _rle_reference(x, piece=None):
    """zlib level 6, strategy Z_RLE, raw: of the whole input, or of independent pieces."""
    if piece is None:
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        return len(co.compress(x) + co.flush())
    return sum(_rle_reference(x[at:at + piece]) for at in range(0, len(x), piece))


@pytest.mark.parametrize("kind", ["smooth", "noise", "banded"])
def test_coder_size_against_zlib_rle(eng, kind):
    from pano360_amd import png
    rgb = banded(256, 192) if kind == "banded" else content(kind, 256, 192)
    x = M.scanlines(rgb).tobytes()
    z = png.deflate_device(x, eng)
    assert zlib.decompress(z) == x
    got, ref = len(z) - 6, _rle_reference(x)
    chunking = _rle_reference(x, png.CHUNK) / ref - 1
    print(f"coder {kind}: device {got}, zlib Z_RLE {ref} ({100 * (got / ref - 1):+.3f} %), "
          f"zlib's own 64 KiB chunking {100 * chunking:+.3f} %, "
          f"beyond it {100 * (got / ref - 1 - chunking):+.3f} %")
    margin = max(chunking, 0.0) + CODER_EXCESS
    assert margin <= 0.03
    assert got <= ref * (1 + margin)


# ---- whole files -------------------------------------------------------------------------------
def _pillow_size(rgb):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "PNG")
    return len(buf.getvalue())


@pytest.mark.parametrize("order", ["rgb", "bgr"])
def test_files_open_in_pillow(eng, order):
    from pano360_amd import png
    for w, h in ((1, 1), (2, 3), (41, 97), (256, 192)):
        for kind in KINDS:
            rgb = content(kind, w, h)
            data = png.encode_device(rgb if order == "rgb" else _bgr(rgb), order, eng)
            back = Image.open(io.BytesIO(data))
            assert back.mode == "RGB" and back.size == (w, h)
            assert np.array_equal(np.asarray(back), rgb), (w, h, kind)
            parts = check_structure(data, w, h)
            assert len(parts) == 1 and zlib.decompress(parts[0]) == M.scanlines(rgb).tobytes()
            assert png.encode_device(rgb if order == "rgb" else _bgr(rgb), order, eng) == data
    rgb = content("noise", 41, 97)
    cut = png.encode_device(rgb, "rgb", eng, idat_bytes=1000)
    parts = check_structure(cut, 41, 97)
    assert len(parts) > 1 and all(len(p) <= 1000 for p in parts)
    assert b"".join(parts) == check_structure(png.encode_device(rgb, "rgb", eng), 41, 97)[0]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(cut))), rgb)


def test_file_of_a_crop_view_and_write(eng, tmp_path):
    import torch
    from pano360_amd import png
    big = content("smooth", 300, 220)
    dev = torch.from_numpy(_bgr(big)).to(eng.device)
    view = dev[9:201, 21:277]
    assert not view.is_contiguous()
    data = png.encode_device(view, eng=eng)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), big[9:201, 21:277])
    assert data == png.encode_device(_bgr(big[9:201, 21:277]), eng=eng)
    assert png.write(str(tmp_path / "a.png"), view, eng=eng) == "device"
    assert (tmp_path / "a.png").read_bytes() == data
    rgba = np.dstack([big, np.full(big.shape[:2], 200, np.uint8)])
    assert png.write(str(tmp_path / "b.png"), rgba, order="rgb", eng=eng) == "pillow"
    assert np.array_equal(np.asarray(Image.open(tmp_path / "b.png")), rgba)


@pytest.mark.parametrize("kind", ["smooth", "banded"])
def test_file_size_against_pillow(eng, kind):
    """A dead filter stage (filter None on every row) gives 1.42 x Pillow's size here."""
    from pano360_amd import png
    rgb = banded(256, 192) if kind == "banded" else content(kind, 256, 192)
    data = png.encode_device(rgb, "rgb", eng)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), rgb)
    pillow = _pillow_size(rgb)
    print(f"file {kind}: device {len(data)}, Pillow {pillow}, ratio {len(data) / pillow:.4f}")
    assert len(data) <= 1.10 * pillow


# ---- the CLI -----------------------------------------------------------------------------------
def test_cli_png_output_takes_the_device_path(eng, tmp_path, monkeypatch):
    import pickle
    import bundle_adj
    import stitcher as top
    from pano360_amd import png, synth
    imgs, rots, intrs = synth.make_scene(5, 200, 120, sweep_deg=80.0, jitter=0.01, seed=9, kind="B")
    regions = [bundle_adj.Image(im, r, k) for im, r, k in zip(imgs, rots, intrs)]
    with open(tmp_path / "ba_RIG_s2.pkl", "wb") as fid:
        pickle.dump(regions, fid, protocol=pickle.HIGHEST_PROTOCOL)
    monkeypatch.chdir(tmp_path)
    calls = []
    real = png.encode_device

    def spy(img, *args, **kwargs):
        calls.append(tuple(img.shape))
        return real(img, *args, **kwargs)

    monkeypatch.setattr(png, "encode_device", spy)
    got = top.main([str(tmp_path / "RIG"), "-b", "linear", "-c", "-o", "m.png"])
    assert calls == [got.shape]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "m.png"))[..., ::-1], got)
    again = top.main([str(tmp_path / "RIG"), "-b", "linear", "-c", "-o", "m.bmp"])
    assert len(calls) == 1 and np.array_equal(again, got)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "m.bmp"))[..., ::-1], got)
