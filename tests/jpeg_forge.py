"""A baseline JPEG writer for tests: streams whose every header and entropy-coding choice is
set by hand, for the parts of ``pano360_amd.jpeg.parse``'s scope that Pillow never writes (SOF1,
grey frames with sampling factors, table slots 2-3, 16-bit DQT, fill bytes, odd component ids,
big-endian EXIF, thumbnails, MPF, trailing bytes) and for Huffman tables far from Annex K.

Pixels go through ``jpeg_encode_model``'s colour conversion, downsampling, ISLOW FDCT and
quantisation with any quantisation tables; quantised blocks can also be given directly.  The
symbols are generated and the bits packed with NumPy, so 4K frames take seconds.  ``forge``
checks every stream it writes: each interval ends with at most 7 one-bits of padding and, for
streams of up to ``CHECK_BLOCKS`` blocks, ``jpeg_model.coefficients`` reads back exactly the
blocks that went in."""
import struct

import numpy as np

import jpeg_encode_model as E
import jpeg_model as M
from pano360_amd import jpeg as J

CHECK_BLOCKS = 6000
SOI, EOI = b"\xff\xd8", b"\xff\xd9"
STD_DC = {0: J.STD_DC_LUMA, 1: J.STD_DC_CHROMA}
STD_AC = {0: J.STD_AC_LUMA, 1: J.STD_AC_CHROMA}
JFIF = b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"


def segment(marker, body, fill=0):
    """One marker segment, preceded by ``fill`` FF fill bytes."""
    return b"\xff" * fill + bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


# ---- geometry and blocks --------------------------------------------------------------------
def geometry(width, height, samp):
    """(MCUs across, MCUs down, the component of each block of an MCU) for the sampling
    factors ``samp`` [(h, v)] of one scan (one component: one block per MCU, T.81 A.2.2)."""
    if len(samp) == 1:
        return -(-width // 8), -(-height // 8), [0]
    hm, vm = max(h for h, _ in samp), max(v for _, v in samp)
    comp_of_u = [c for c, (h, v) in enumerate(samp) for _ in range(h * v)]
    return -(-width // (8 * hm)), -(-height // (8 * vm)), comp_of_u


def _quantized(plane, q):
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    p = plane.reshape(bh, 8, bw, 8).swapaxes(1, 2).reshape(-1, 8, 8)
    return E.quantize(E.fdct_islow(p).reshape(-1, 64), np.asarray(q)).reshape(bh, bw, 64)


def image_blocks(img, samp, qts):
    """Quantised blocks (int32 [blocks][64], natural order, MCU order, DC absolute) of a uint8
    image: RGB [h][w][3] for YCbCr 4:4:4 / 4:2:2 / 4:2:0 ``samp``, or grey [h][w] (or the luma
    of an RGB image) for one component.  ``qts``: the quantisation table (natural order) of
    each component."""
    height, width = img.shape[:2]
    mx, my, _ = geometry(width, height, samp)
    if len(samp) == 1:
        g = img if img.ndim == 2 else E.rgb_to_ycc(img)[0]
        rows = np.minimum(np.arange(8 * my), height - 1)
        cols = np.minimum(np.arange(8 * mx), width - 1)
        return _quantized(np.asarray(g, np.int64)[rows][:, cols], qts[0]).reshape(-1, 64) \
            .astype(np.int32)
    sub = {(1, 1): 0, (2, 1): 1, (2, 2): 2}[tuple(samp[0])]
    assert [tuple(s) for s in samp[1:]] == [(1, 1), (1, 1)]
    parts = []
    for c, (plane, (h, v)) in enumerate(zip(E.planes(img, sub), samp)):
        grid = _quantized(plane, qts[c])                  # [my * v][mx * h][64]
        parts.append(grid.reshape(my, v, mx, h, 64).transpose(0, 2, 1, 3, 4)
                     .reshape(my * mx, v * h, 64))
    return np.concatenate(parts, axis=1).reshape(-1, 64).astype(np.int32)


# ---- symbols ----------------------------------------------------------------------------------
def _magnitude(v):
    """(size category, the value's bits) of T.81 F.1.2.1, vectorised."""
    v = np.asarray(v, np.int64)
    n = np.frexp(np.abs(v).astype(np.float64))[1].astype(np.int64)
    return n, np.where(v >= 0, v, v - 1) & ((np.int64(1) << n) - 1)


# event kinds: a DC symbol, an AC symbol, raw bits
DC_SYM, AC_SYM, RAW = 0, 1, 2


def symbols(blocks, comp_of_u, restart, td, ta):
    """The scan as events in stream order: (kind, table slot, symbol or raw bits, raw length,
    interval).  DC prediction restarts with every interval (``restart`` MCUs, 0: one)."""
    blocks = np.asarray(blocks, np.int64)
    nb, bpm = len(blocks), len(comp_of_u)
    zz = blocks[:, J.ZIGZAG]
    comp = np.tile(np.asarray(comp_of_u), nb // bpm)
    interval = (np.arange(nb) // bpm) // restart if restart else np.zeros(nb, np.int64)
    dc = zz[:, 0]
    diff = np.empty(nb, np.int64)
    for c in set(comp_of_u):
        idx = np.nonzero(comp == c)[0]
        prev = np.r_[0, dc[idx][:-1]]
        prev[np.r_[True, interval[idx][1:] != interval[idx][:-1]]] = 0
        diff[idx] = dc[idx] - prev
    ac = zz[:, 1:]
    bi, ki = np.nonzero(ac)
    k = ki + 1
    first = np.r_[True, bi[1:] != bi[:-1]] if len(bi) else np.zeros(0, bool)
    prevk = np.r_[0, k[:-1]] if len(k) else k
    prevk = np.where(first, 0, prevk)
    run = k - prevk - 1
    nnz = np.bincount(bi, minlength=nb)
    lastk = np.zeros(nb, np.int64)
    ends = np.cumsum(nnz) - 1
    lastk[nnz > 0] = k[ends[nnz > 0]]
    # per block: DC symbol, DC bits, 5 slots per nonzero (3 ZRL, symbol, bits), EOB
    count = 3 + 5 * nnz
    start = np.cumsum(count) - count
    total = int(count.sum())
    kind = np.full(total, RAW, np.int8)
    tab = np.zeros(total, np.int8)
    val = np.zeros(total, np.int64)
    rlen = np.zeros(total, np.int64)
    tdc = np.asarray(td)[comp]
    tac = np.asarray(ta)[comp]
    n, bits = _magnitude(diff)
    kind[start], tab[start], val[start] = DC_SYM, tdc, n
    val[start + 1], rlen[start + 1] = bits, n
    if len(bi):
        rank = np.arange(len(bi)) - (np.cumsum(nnz) - nnz)[bi]
        base = start[bi] + 2 + 5 * rank
        for z in range(3):
            sel = run // 16 > z
            kind[base[sel] + z], tab[base[sel] + z], val[base[sel] + z] = AC_SYM, tac[bi][sel], 0xF0
        s, b = _magnitude(ac[bi, ki])
        kind[base + 3], tab[base + 3], val[base + 3] = AC_SYM, tac[bi], ((run % 16) << 4) | s
        val[base + 4], rlen[base + 4] = b, s
    eob = lastk < 63
    e = start + count - 1
    kind[e[eob]], tab[e[eob]], val[e[eob]] = AC_SYM, tac[eob], 0x00
    keep = (kind != RAW) | (rlen > 0)
    return (kind[keep], tab[keep], val[keep], rlen[keep],
            np.repeat(interval, count)[keep])


def frequencies(ev, kind, slot):
    k, t, v = ev[:3]
    return np.bincount(v[(k == kind) & (t == slot)], minlength=256)[:256]


# ---- Huffman tables -----------------------------------------------------------------------------
def optimal_table(freq):
    """libjpeg's ``jpeg_gen_optimal_table`` (jchuff.c), restated: a Huffman code of the
    frequencies with a reserved all-ones code point, limited to 16 bits."""
    freq = [int(f) for f in freq[:256]] + [1]
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        v = 1 << 62
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        v = 1 << 62
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [j for size in range(1, 33) for j in range(256) if codesize[j] == size]
    return bits[1:17], bytes(vals)


def _by_length(lengths):
    """(BITS, HUFFVAL) of {symbol: code length}; symbols of one length keep the dict's order."""
    bits = [0] * 16
    vals = []
    for length in range(1, 17):
        for sym, l in lengths.items():
            if l == length:
                bits[length - 1] += 1
                vals.append(sym)
    return bits, bytes(vals)


def _used(freq):
    return [int(s) for s in np.argsort(-np.asarray(freq), kind="stable") if freq[s] > 0]


def deep_table(freq):
    """Every used symbol gets a code of 10 to 16 bits (none reaches the 9-bit fast table)."""
    used = _used(freq)
    step = max(1, -(-len(used) // 7))
    return _by_length({s: 10 + i // step for i, s in enumerate(used)})


def ff_dense_table(freq, dc):
    """Codes made mostly of ones for the symbols in use: unused symbols take the codes 0, 10,
    110, ... (as many as the 16-bit limit leaves room for), and the used ones share the rest under
    that all-ones prefix, the most frequent one last, i.e. with the most ones."""
    used = _used(freq)
    spare = [s for s in range(16 if dc else 256) if s not in used]
    q = max(1, int(len(used)).bit_length())             # 2^q - 1 >= len(used): no all-ones
    p = min(16 - q, len(spare))
    lengths = {spare[i]: i + 1 for i in range(p)}
    lengths.update({s: p + q for s in reversed(used)})
    return _by_length(lengths)


def minimal_table(sym):
    return [1] + [0] * 15, bytes([sym])


def make_table(spec, freq, dc, slot=0):
    if spec == "std":
        return (STD_DC if dc else STD_AC)[min(slot, 1)]
    if spec == "optimal":
        return optimal_table(freq)
    if spec == "deep":
        return deep_table(freq)
    if spec == "ffdense":
        return ff_dense_table(freq, dc)
    if spec == "minimal":
        used = _used(freq)
        assert len(used) == 1, used
        return minimal_table(used[0])
    return spec                                         # (BITS, HUFFVAL) given as is


# ---- the entropy-coded segment ------------------------------------------------------------------
def _lookup(tables):
    code = np.zeros((2, 4, 256), np.int64)
    size = np.zeros((2, 4, 256), np.int64)
    for (kind, slot), (bits, vals) in tables.items():
        for length, c, sym in J.huff_codes(bits, vals):
            code[kind, slot, sym], size[kind, slot, sym] = c, length
    return code, size


def entropy_segment(ev, tables, nint, rst_fill=0):
    """The entropy-coded bytes: each interval's bits padded with ones to a byte, stuffed, then
    RSTn (after ``rst_fill`` fill bytes) between intervals.  Returns (bytes, [padding bits of
    each interval])."""
    kind, tab, val, rlen, iv = ev
    code, size = _lookup(tables)
    sym = kind != RAW
    ki, ti, vi = kind[sym].astype(np.int64), tab[sym].astype(np.int64), val[sym]
    assert (size[ki, ti, vi] > 0).all(), "a symbol missing from its Huffman table"
    length = rlen.copy()
    word = val.copy()
    length[sym] = size[ki, ti, vi]
    word[sym] = code[ki, ti, vi]
    per = np.bincount(iv, weights=length, minlength=nint).astype(np.int64)
    padded = (per + 7) // 8 * 8
    pad = padded - per
    assert (pad <= 7).all()
    ustart = np.cumsum(per) - per
    pstart = np.cumsum(padded) - padded
    excl = np.cumsum(length) - length
    pos = pstart[iv] + excl - ustart[iv]
    bits = np.ones(int(padded.sum()), np.uint8)
    rep_len = np.repeat(length, length)
    j = np.arange(int(length.sum()), dtype=np.int64) - np.repeat(excl, length)
    bits[np.repeat(pos, length) + j] = (np.repeat(word, length) >> (rep_len - 1 - j)) & 1
    raw = np.packbits(bits).tobytes()
    out = []
    bstart = pstart // 8
    for i in range(nint):
        out.append(raw[bstart[i]:bstart[i] + padded[i] // 8].replace(b"\xff", b"\xff\x00"))
        if i + 1 < nint:
            out.append(b"\xff" * rst_fill + bytes([0xFF, 0xD0 + i % 8]))
    return b"".join(out), pad.tolist()


# ---- APP segments ------------------------------------------------------------------------------
def exif(orientation=1, order="II", thumbnail=None, orient_type=3):
    """An APP1 EXIF body: IFD0 with the orientation (SHORT, or ``orient_type``), and IFD1
    pointing at an embedded JPEG thumbnail when one is given."""
    e = "<" if order == "II" else ">"
    head = order.encode() + struct.pack(e + "HI", 42, 8)
    entries = [(0x0112, orient_type, 1,
                struct.pack(e + "HH", orientation, 0) if orient_type == 3
                else struct.pack(e + "I", orientation))]
    ifd0_len = 2 + 12 * len(entries) + 4
    ifd1_off = 8 + ifd0_len if thumbnail is not None else 0
    ifd0 = struct.pack(e + "H", len(entries)) + b"".join(
        struct.pack(e + "HHI", t, ty, n) + v for t, ty, n, v in entries) + \
        struct.pack(e + "I", ifd1_off)
    body = head + ifd0
    if thumbnail is not None:
        thumb_off = ifd1_off + 2 + 2 * 12 + 4
        body += struct.pack(e + "H", 2) + \
            struct.pack(e + "HHII", 0x0201, 4, 1, thumb_off) + \
            struct.pack(e + "HHII", 0x0202, 4, 1, len(thumbnail)) + struct.pack(e + "I", 0) + \
            thumbnail
    return b"Exif\0\0" + body


def mpf():
    """An APP2 MPF body (CIPA DC-007) indexing two images, without its 32 bytes of MP entries
    (``_mp_entries``, which ``forge`` fills in once the file's length is known)."""
    e = "<"
    n = 3
    ifd = struct.pack(e + "H", n)
    ifd += struct.pack(e + "HHI", 0xB000, 7, 4) + b"0100"
    ifd += struct.pack(e + "HHII", 0xB001, 4, 1, 2)
    entries_off = 8 + 2 + 12 * n + 4
    ifd += struct.pack(e + "HHII", 0xB002, 7, 32, entries_off)
    ifd += struct.pack(e + "I", 0)
    return b"MPF\0" + b"II*\0" + struct.pack(e + "I", 8) + ifd


def _mp_entries(first_len, second_len, second_off):
    return (struct.pack("<IIIHH", 0x20030000, first_len, 0, 0, 0) +
            struct.pack("<IIIHH", 0x00000000, second_len, second_off, 0, 0))


# ---- the file ------------------------------------------------------------------------------------
class Forged:
    """A forged stream: ``blob``, the blocks that went in (DC absolute), its header as
    ``parse`` reads it, and facts the tests check coverage against."""

    def __init__(self, blob, blocks, pad, nint, tables):
        self.blob, self.blocks, self.pad, self.nint, self.tables = blob, blocks, pad, nint, tables
        self.hdr = J.parse(blob)

    @property
    def entropy(self):
        return self.blob[self.hdr.data_start:self.hdr.data_end]


def forge(width, height, blocks, comps, qts, dc="std", ac="std", *, sof=0xC0, restart=0,
          dri=None, dri_after_dht=False, table_segments="one", dqt16=False, redefine=False,
          app0=True, apps=(), exif_body=None, fill=0, rst_fill=0, eoi_fill=0, mpf_second=None,
          trailer=b"", check=True):
    """A baseline JPEG of quantised ``blocks`` (``image_blocks``' layout).

    comps: [(id, h, v, tq, td, ta)]; qts: {slot: int[64] natural order}; dc / ac: a table spec
    ("std", "optimal", "deep", "ffdense", "minimal" or (BITS, HUFFVAL)) per used slot, or one
    spec for all.  restart: the interval in MCUs written into DRI (``dri`` overrides what is
    written: 0 writes an explicit DRI of 0); table_segments: "one" (every table in one DQT and
    one DHT) or "each"; redefine: each table is first defined with other content, then again;
    apps: extra (marker, body) segments after APP0; fill / rst_fill / eoi_fill: FF fill bytes
    before every header marker, every RSTn, EOI; mpf_second: a JPEG appended after EOI and
    indexed by an APP2 MPF segment; trailer: bytes after everything."""
    samp = [(c[1], c[2]) for c in comps]
    mx, my, comp_of_u = geometry(width, height, samp)
    nmcu = mx * my
    blocks = np.asarray(blocks, np.int32)
    assert blocks.shape == (nmcu * len(comp_of_u), 64), (blocks.shape, nmcu, comp_of_u)
    q = np.stack([np.asarray(qts[comps[c][3]]) if comps[c][3] in qts else np.ones(64)
                  for c in range(len(comps))]).astype(np.int64)
    ctab = np.tile(np.asarray(comp_of_u), nmcu)
    assert (np.abs(blocks.astype(np.int64) * q[ctab]) < 1 << 15).all(), \
        "dequantised coefficients beyond 16 bits"
    td = [c[4] for c in comps]
    ta = [c[5] for c in comps]
    ev = symbols(blocks, comp_of_u, restart, td, ta)
    nint = -(-nmcu // restart) if restart else 1
    tables = {}
    for kind, slots, spec in ((DC_SYM, sorted(set(td)), dc), (AC_SYM, sorted(set(ta)), ac)):
        for s in slots:
            sp = spec[s] if isinstance(spec, dict) else spec
            tables[(kind, s)] = make_table(sp, frequencies(ev, kind, s), kind == DC_SYM, s)
    data, pad = entropy_segment(ev, tables, nint, rst_fill)

    def f(marker, body):
        return segment(marker, body, fill)

    head = [SOI]
    if app0:
        head.append(f(0xE0, JFIF))
    if exif_body is not None:
        head.append(f(0xE1, exif_body))
    mpf_at = None
    if mpf_second is not None:
        mpf_at = len(b"".join(head))
        head.append(f(0xE2, mpf() + bytes(32)))
    for marker, body in apps:
        head.append(f(marker, body))
    dri_seg = f(0xDD, (restart if dri is None else dri).to_bytes(2, "big")) \
        if (restart or dri is not None) else b""
    if not dri_after_dht:
        head.append(dri_seg)
    qparts = []
    for slot in sorted(qts):
        q = np.asarray(qts[slot])[J.ZIGZAG]
        body = q.astype(">u2").tobytes() if dqt16 else q.astype(np.uint8).tobytes()
        qparts.append(bytes([(0x10 if dqt16 else 0) | slot]) + body)
    hparts = []
    for (kind, slot), (bits, vals) in sorted(tables.items()):
        hparts.append(bytes([kind << 4 | slot] + list(bits)) + bytes(vals))
    if redefine:                                        # first a wrong table, then the real one
        wq = [bytes([p[0]]) + bytes([1] * 64) for p in qparts if not dqt16] or \
            [bytes([p[0]]) + np.ones(64, ">u2").tobytes() for p in qparts]
        wh = [bytes([p[0]]) + bytes(J.STD_DC_CHROMA[0]) + J.STD_DC_CHROMA[1] for p in hparts]
        head += [f(0xDB, b"".join(wq)), f(0xC4, b"".join(wh))]
    sof_body = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + \
        bytes([len(comps)]) + b"".join(bytes([c[0], c[1] << 4 | c[2], c[3]]) for c in comps)
    if table_segments == "one":
        head.append(f(0xDB, b"".join(qparts)))
        head.append(f(sof, sof_body))
        head.append(f(0xC4, b"".join(hparts)))
    else:
        head += [f(0xDB, p) for p in qparts]
        head.append(f(sof, sof_body))
        head += [f(0xC4, p) for p in hparts]
    if dri_after_dht:
        head.append(dri_seg)
    head.append(f(0xDA, bytes([len(comps)]) + b"".join(bytes([c[0], c[4] << 4 | c[5]])
                                                       for c in comps) + bytes([0, 63, 0])))
    blob = b"".join(head) + data + b"\xff" * eoi_fill + EOI
    if mpf_second is not None:                          # fill in the MP index
        body = mpf()
        mp_header = mpf_at + fill + 4 + 4                 # FF E2 len "MPF\0" -> the TIFF header
        entries = _mp_entries(len(blob), len(mpf_second), len(blob) - mp_header)
        seg_body_at = mpf_at + fill + 4
        b = bytearray(blob)
        b[seg_body_at + len(body):seg_body_at + len(body) + 32] = entries
        blob = bytes(b) + mpf_second
    blob += trailer
    out = Forged(blob, blocks, pad, nint, tables)
    assert out.hdr is not None or not check, "parse() rejects a stream meant to be in scope"
    if check and out.hdr is not None and len(blocks) <= CHECK_BLOCKS:
        got = M.coefficients(out.hdr, blob)
        assert np.array_equal(got, blocks), "the model reads back other blocks"
    return out
