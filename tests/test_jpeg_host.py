"""Host side of the device JPEG decode: the NumPy model (tests/jpeg_model.py) equals Pillow bit
for bit, the marker parser accepts exactly the baseline subset, and the packed batch layout
agrees with include/pano360.h.  Every image is made with Pillow here."""
import io
import os
import re

import numpy as np
import pytest
from PIL import Image, ImageOps

import jpeg_model as M
from pano360_amd import jpeg as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLING = {"444": 0, "422": 1, "420": 2}
SIZES = [(1, 1), (2, 5), (7, 9), (17, 33), (33, 17)]


def make(w, h, mode="RGB", seed=0, noise=False, orientation=None, **kw):
    """Pillow-encoded JPEG bytes of a w x h image (a smooth pattern plus noise, or pure noise)."""
    rng = np.random.default_rng(seed + 7919 * w + h)
    if noise:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 255 // max(w, 1), yy * 255 // max(h, 1), (xx + yy) * 7 % 256], -1)
        a = np.clip(base + rng.integers(-30, 30, (h, w, 3)), 0, 255).astype(np.uint8)
    im = Image.fromarray(a)
    if mode == "L":
        im = im.convert("L")
    if orientation is not None:
        exif = Image.Exif()
        exif[0x0112] = orientation
        kw["exif"] = exif.tobytes()
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow(blob):
    im = ImageOps.exif_transpose(Image.open(io.BytesIO(blob)))
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def matrix():
    """(id, blob) of the decode matrix shared with tests/test_gpu_jpeg.py."""
    out = []
    for w, h in SIZES:
        for samp in ("444", "422", "420", "grey"):
            for q in (10, 75, 95, 100):
                kw = dict(quality=q)
                mode = "L" if samp == "grey" else "RGB"
                if mode == "RGB":
                    kw["subsampling"] = SAMPLING[samp]
                out.append((f"{w}x{h}-{samp}-q{q}", make(w, h, mode, noise=q == 100, **kw)))
    for samp in ("444", "422", "420", "grey"):
        mode = "L" if samp == "grey" else "RGB"
        kw = {} if mode == "L" else {"subsampling": SAMPLING[samp]}
        out.append((f"opt-{samp}", make(33, 17, mode, optimize=True, quality=85, **kw)))
        out.append((f"rstblk-{samp}", make(40, 27, mode, restart_marker_blocks=1, **kw)))
        out.append((f"rstrow-{samp}", make(35, 41, mode, restart_marker_rows=1, **kw)))
        out.append((f"rst3-{samp}", make(64, 48, mode, restart_marker_blocks=3, optimize=True,
                                          **kw)))
    for o in range(1, 9):
        out.append((f"orient{o}-420", make(17, 10, orientation=o, subsampling=2)))
        out.append((f"orient{o}-grey", make(9, 6, "L", orientation=o)))
    return out


MATRIX = matrix()


@pytest.mark.parametrize("blob", [b for _, b in MATRIX], ids=[i for i, _ in MATRIX])
def test_model_equals_pillow(blob):
    hdr = J.parse(blob)
    assert hdr is not None
    got = M.decode(blob, hdr)
    want = pillow(blob)
    assert got.shape == want.shape and np.array_equal(got, want)


def test_range_limit_is_the_ten_bit_table():
    v = np.arange(-2048, 2048)
    table = np.zeros(1024, np.int64)             # libjpeg's post-IDCT table, entry (v & 1023)
    table[:128] = np.arange(128, 256)
    table[128:512] = 255
    table[512:896] = 0
    table[896:] = np.arange(0, 128)
    assert np.array_equal(M.range_limit(v), table[v & 1023])


def _progressive():
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, "JPEG", progressive=True)
    return buf.getvalue()


def _cmyk():
    buf = io.BytesIO()
    Image.new("CMYK", (16, 16), (1, 2, 3, 4)).save(buf, "JPEG")
    return buf.getvalue()


def _adobe_rgb():
    """A 3-component baseline file with an Adobe APP14 segment (transform 0: RGB)."""
    blob = make(16, 16)
    app14 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    return blob[:2] + app14 + blob[2:]


def test_parser_accepts_the_baseline_subset():
    for name, blob in MATRIX:
        hdr = J.parse(blob)
        assert hdr is not None, name
        assert blob[hdr.data_end:hdr.data_end + 2] == b"\xff\xd9"
    hdr = J.parse(make(17, 33, subsampling=2))
    assert (hdr.width, hdr.height, hdr.mcus) == (17, 33, (2, 3, 6))
    assert [c[1:3] for c in hdr.comps] == [(2, 2), (1, 1), (1, 1)]
    assert J.parse(make(17, 33, subsampling=1)).mcus == (2, 5, 4)
    assert J.parse(make(17, 33, "L")).mcus == (3, 5, 1)
    assert J.parse(make(40, 27, restart_marker_blocks=1)).restart == 1
    assert J.parse(make(9, 6, orientation=6)).out_shape == (9, 6)


def _coarse_quant():
    """A 16-bit DQT table with quantisers above 255 (beyond the bit-exact IDCT range)."""
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, "JPEG",
                                                          qtables=[[300] * 64, [2] * 64])
    return buf.getvalue()


@pytest.mark.parametrize("kind", ["progressive", "truncated", "cmyk", "adobe-rgb", "png",
                                  "no-eoi", "empty", "quant-300"])
def test_parser_rejects_everything_else(kind):
    blob = {"progressive": _progressive, "cmyk": _cmyk, "adobe-rgb": _adobe_rgb,
            "truncated": lambda: make(64, 48)[:300],
            "no-eoi": lambda: make(64, 48)[:-2],
            "empty": lambda: b"",
            "png": lambda: _png(), "quant-300": _coarse_quant}[kind]()
    assert J.parse(blob) is None


def _png():
    buf = io.BytesIO()
    Image.new("RGB", (4, 4)).save(buf, "PNG")
    return buf.getvalue()


def test_huffman_lookup_table_decodes_every_code():
    hdr = J.parse(make(33, 17, optimize=True))
    for bits, vals in [t for t in hdr.dc + hdr.ac if t is not None]:
        tab = J.huff_table(bits, vals)
        assert len(tab) == J.HUFF_BYTES
        fast = np.frombuffer(tab[:1024], np.uint16)
        maxcode = np.frombuffer(tab[1024:1096], np.int32)
        valoff = np.frombuffer(tab[1096:1168], np.int32)
        v = np.frombuffer(tab[1168:], np.uint8)
        for length, code, sym in J.huff_codes(bits, vals):
            word = code << (16 - length)
            f = fast[word >> 7]
            if length <= 9:
                assert (f >> 8, f & 255) == (length, sym)
            else:
                assert f == 0
                got = next(l for l in range(10, 17) if (word >> (16 - l)) <= maxcode[l])
                assert got == length and v[valoff[length] + code] == sym


def test_layout_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "pano360.h")).read()
    for macro, value in (("PANO_JPEG_FIELDS", J.JD_FIELDS), ("PANO_JPEG_CHUNK", J.CHUNK),
                         ("PANO_JPEG_SUBSEQ", J.SUBSEQ), ("PANO_JPEG_HUFF_BYTES", J.HUFF_BYTES)):
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value
    for prefix in ("JD", "JB"):
        body = re.search(r"enum \{  /\* %s \*/(.*?)\};" % ("image row" if prefix == "JD"
                                                           else "batch row"), header, re.S)
        names = re.findall(rf"PANO_{prefix}_([A-Z0-9_]+)", re.sub(r"/\*.*?\*/", "",
                                                                   body.group(1), flags=re.S))
        assert [getattr(J, f"{prefix}_{n}") for n in names] == list(range(len(names)))


def test_packed_batch_layout():
    blobs = [make(17, 33, subsampling=2), make(40, 27, "L", restart_marker_blocks=1),
             make(33, 17, subsampling=0, restart_marker_rows=1, orientation=6)]
    headers = [J.parse(b) for b in blobs]
    desc, layout, packed_bytes = J.pack(headers, blobs)
    n = len(blobs)
    bt = desc[n]
    assert bt[J.JB_N] == n and bt[J.JB_PACKED_BYTES] == packed_bytes
    buf = np.zeros(packed_bytes, np.uint8)
    J.fill_packed(buf, desc, layout, headers, blobs)
    assert np.array_equal(buf[:desc.nbytes].view(np.int64).reshape(desc.shape), desc)
    first = dict(chunks=0, ints=0, subs=0, blocks=0, pixels=0)
    spans = []
    for i, (hdr, blob) in enumerate(zip(headers, blobs)):
        d = desc[i]
        mx, my, bpm = hdr.mcus
        data = blob[hdr.data_start:hdr.data_end]
        assert bytes(buf[d[J.JD_DATA_OFF]:d[J.JD_DATA_OFF] + d[J.JD_DATA_LEN]]) == data
        tab = bytes(buf[d[J.JD_TAB_OFF]:d[J.JD_TAB_OFF] + J.TAB_BYTES])
        td = hdr.comps[0][4]
        assert tab[td * J.HUFF_BYTES:(td + 1) * J.HUFF_BYTES] == J.huff_table(*hdr.dc[td])
        q = np.frombuffer(tab[8 * J.HUFF_BYTES:], np.uint16).reshape(4, 64)
        assert np.array_equal(q[hdr.comps[0][3]], hdr.qt[hdr.comps[0][3]])
        assert (d[J.JD_CHUNK0], d[J.JD_INT0], d[J.JD_SUB0], d[J.JD_BLK0], d[J.JD_PIX0]) == \
            tuple(first.values())
        nint = 1 if not hdr.restart else -(-mx * my // hdr.restart)
        assert d[J.JD_NINT] == nint
        first["chunks"] += max(1, -(-len(data) // J.CHUNK))
        first["ints"] += nint
        first["subs"] += len(data) * 8 // J.SUBSEQ + nint + 1
        first["blocks"] += mx * my * bpm
        first["pixels"] += hdr.width * hdr.height
        order = M.block_order(hdr)
        for u in range(bpm):
            assert (d[J.JD_COMP_U] >> (2 * u)) & 3 == order[u][0]
        spans.append((d[J.JD_DST_OFF], d[J.JD_DST_OFF] + len(data)))
        for c in range(len(hdr.comps)):
            h, v = (hdr.comps[c][1], hdr.comps[c][2]) if len(hdr.comps) == 3 else (1, 1)
            assert d[J.JD_PITCH0 + c] == 8 * mx * h
            spans.append((d[J.JD_PLANE0 + c], d[J.JD_PLANE0 + c] + 64 * mx * h * my * v))
    assert [bt[f] for f in (J.JB_CHUNKS, J.JB_INTS, J.JB_SUBS, J.JB_BLOCKS, J.JB_PIXELS)] == \
        list(first.values())
    sizes = {J.JB_W_KEPT: 4 * bt[J.JB_CHUNKS], J.JB_W_STATE0: 16 * bt[J.JB_SUBS],
             J.JB_W_COEF: 128 * bt[J.JB_BLOCKS], J.JB_W_CNTX: 4 * bt[J.JB_SUBS]}
    spans += [(bt[f], bt[f] + s) for f, s in sizes.items()]
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "scratch arrays overlap"
    assert spans[-1][1] <= bt[J.JB_WORK_BYTES]
    outs = [(desc[i, J.JD_OUT_OFF], desc[i, J.JD_OUT_OFF] + 3 * h.width * h.height)
            for i, h in enumerate(headers)]
    assert all(a[1] <= b[0] for a, b in zip(outs, outs[1:]))
    assert outs[-1][1] <= bt[J.JB_OUT_BYTES]


def test_batches_stay_within_the_budgets():
    blobs = [make(64 + 8 * k, 40 + 3 * k, "L" if k % 3 == 0 else "RGB", seed=k, noise=k % 2 == 1,
                  subsampling=k % 3) for k in range(12)]
    headers = [J.parse(b) for b in blobs]
    sizes = [J.pack([h], [b])[2] for h, b in zip(headers, blobs)]
    works = [int(J.pack([h], [b])[0][1, J.JB_WORK_BYTES]) for h, b in zip(headers, blobs)]
    max_packed = (sorted(sizes)[-2] + max(sizes)) // 2    # the largest image alone is too big
    assert sorted(sizes)[-2] < max_packed < max(sizes)
    max_work = 3 * max(works)
    batches, rejected = J.plan_batches(headers, max_packed, max_work)
    assert rejected == [sizes.index(max(sizes))]
    assert len(batches) > 2
    flat = [i for b in batches for i in b]
    assert flat == sorted(flat) and sorted(flat + rejected) == list(range(len(blobs)))
    for b in batches:
        desc, _, packed = J.pack([headers[i] for i in b], [blobs[i] for i in b])
        assert packed <= max_packed and desc[len(b), J.JB_WORK_BYTES] <= max_work
    # greedy: a batch closes only when the next image would not fit in it
    for b, nxt in zip(batches, batches[1:]):
        grown = b + nxt[:1]
        desc, _, packed = J.pack([headers[i] for i in grown], [blobs[i] for i in grown])
        assert packed > max_packed or desc[len(grown), J.JB_WORK_BYTES] > max_work
    # an image over the per-image data limit fits no batch
    lens = [h.data_end - h.data_start for h in headers]
    batches, rejected = J.plan_batches(headers, max_data=max(lens) - 1)
    assert rejected == [lens.index(max(lens))] and len(batches) == 1
    assert J.plan_batches(headers) == ([list(range(len(blobs)))], [])
    with pytest.raises(ValueError):
        J.plan_batches(headers, max_packed=1 << 31)
