"""Baseline JPEG decode on the device (``pano_jpeg_decode``, csrc/jpeg.hip).

``parse`` reads the markers of one file on the host and returns a ``Header``, or None for
anything the device path does not cover: progressive, arithmetic, lossless or 12-bit files,
more than one scan, CMYK / YCCK / Adobe-transform files, sampling other than 4:4:4, 4:2:2 and
4:2:0, quantisers above 255, XMP orientation, Huffman tables libjpeg refuses, and every truncated or
inconsistent file.  Those go to Pillow.

``pack`` lays a batch out as the native call expects it (the layout is documented at
``pano_jpeg_decode`` in include/pano360.h): one int64 descriptor table, the per-image Huffman
and quantisation tables, the entropy-coded bytes, and the offsets of every scratch array.
``decode_device`` uploads that in one copy and decodes the whole batch in one call; the frames
equal ``ImageOps.exif_transpose(Image.open(f)).convert("RGB")`` bit for bit, in BGR order.
``read_images`` routes each file to the device or to Pillow and says which path it took; it cuts
the device's share into batches within the native limits and a memory budget (``plan_batches``).
"""
import ctypes as C
import os
import re

import numpy as np

from . import _lib

# natural-order index of the k-th zigzag coefficient (ITU-T T.81 figure A.6)
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int32)

# ---- the native layout (include/pano360.h, pano_jpeg_decode) ----------------------------------
# per-image descriptor fields (int64 each)
(JD_W, JD_H, JD_NC, JD_HMAX, JD_VMAX, JD_MCUX, JD_MCUY, JD_RI, JD_NINT, JD_BPM, JD_ORIENT,
 JD_DATA_OFF, JD_DATA_LEN, JD_TAB_OFF, JD_CHUNK0, JD_INT0, JD_SUB0, JD_BLK0, JD_PIX0,
 JD_DST_OFF, JD_PLANE0, JD_PLANE1, JD_PLANE2, JD_PITCH0, JD_PITCH1, JD_PITCH2, JD_OUT_OFF,
 JD_COMP_U, JD_SAMP, JD_TABSEL) = range(30)
JD_FIELDS = _lib.JPEG_FIELDS
# batch row (after the n image rows): totals and the scratch arrays' offsets in `work`
(JB_N, JB_CHUNKS, JB_INTS, JB_SUBS, JB_BLOCKS, JB_PIXELS, JB_OUT_BYTES, JB_W_KEPT, JB_W_RST,
 JB_W_KEPTX, JB_W_RSTX, JB_W_DSTLEN, JB_W_ISTART, JB_W_IEND, JB_W_INSUB, JB_W_ISUBX, JB_W_STATE0,
 JB_W_STATE1, JB_W_CNTX, JB_W_FLAG, JB_W_COEF, JB_WORK_BYTES, JB_PACKED_BYTES) = range(23)
CHUNK = _lib.JPEG_CHUNK             # raw entropy bytes per destuffing thread
SUBSEQ = _lib.JPEG_SUBSEQ           # bits per Huffman subsequence
# one lookup table: fast[512] u16, maxcode[18] i32, valoff[18] i32, vals[256]
HUFF_BYTES = _lib.JPEG_HUFF_BYTES
TAB_BYTES = 8 * HUFF_BYTES + 4 * 64 * 2     # 4 DC + 4 AC tables, then 4 quantisation tables
# Quantisers above 255 (16-bit DQT tables) go to Pillow: with them the dequantised coefficients
# can leave 16 bits, where libjpeg-turbo's C IDCT (64-bit) and its SIMD IDCT (16-bit products,
# what Pillow runs) already disagree, and the device's int32 IDCT matches neither.
MAX_QUANT = 255
# Native limits (pano_jpeg_decode): entropy bytes of one image, packed bytes of one batch
MAX_IMAGE_DATA = (1 << 28) - 1
MAX_PACKED = (1 << 31) - 1
# read_images' batch budget: packed (compressed) bytes and scratch bytes per native call
BATCH_PACKED = 1 << 30
BATCH_WORK = 8 << 30


class Header:
    """What the device needs of one in-scope file."""
    __slots__ = ("width", "height", "comps", "qt", "dc", "ac", "restart", "orientation",
                 "data_start", "data_end")

    @property
    def hmax(self):
        return max(c[1] for c in self.comps)

    @property
    def vmax(self):
        return max(c[2] for c in self.comps)

    @property
    def mcus(self):
        """(MCUs across, MCUs down, blocks per MCU).  One component: one block per MCU."""
        if len(self.comps) == 1:
            return -(-self.width // 8), -(-self.height // 8), 1
        return (-(-self.width // (8 * self.hmax)), -(-self.height // (8 * self.vmax)),
                sum(c[1] * c[2] for c in self.comps))

    @property
    def out_shape(self):
        return (self.width, self.height) if self.orientation >= 5 else (self.height, self.width)


def _exif_orientation(s):
    """EXIF orientation of an APP1 payload after b"Exif\\0\\0"; None if it cannot be read the
    way Pillow would."""
    if len(s) < 8 or s[:2] not in (b"II", b"MM"):
        return None
    e = "<" if s[:2] == b"II" else ">"
    if int.from_bytes(s[2:4], "little" if e == "<" else "big") != 42:
        return None
    rd = (lambda o, n: int.from_bytes(s[o:o + n], "little" if e == "<" else "big"))
    ifd = rd(4, 4)
    if ifd + 2 > len(s):
        return None
    count = rd(ifd, 2)
    if ifd + 2 + 12 * count > len(s):
        return None
    for i in range(count):
        o = ifd + 2 + 12 * i
        if rd(o, 2) == 0x0112:
            if rd(o + 2, 2) != 3 or rd(o + 4, 4) != 1:
                return None
            v = rd(o + 8, 2)
            return v if 1 <= v <= 8 else 1
    return 1


_MARKER_END = re.compile(rb"\xff[^\x00\xd0-\xd7\xff]")


def parse(blob):
    """The header of a baseline JPEG the device decodes, or None (see the module docstring)."""
    b = bytes(blob) if not isinstance(blob, (bytes, bytearray)) else blob
    n = len(b)
    if n < 4 or b[0] != 0xFF or b[1] != 0xD8:
        return None
    qt, dc, ac = [None] * 4, [None] * 4, [None] * 4
    sof, restart, orientation, exif_seen = None, 0, 1, False
    pos = 2
    while True:
        while pos < n and b[pos] == 0xFF and pos + 1 < n and b[pos + 1] == 0xFF:
            pos += 1                                    # fill bytes before a marker
        if pos + 4 > n or b[pos] != 0xFF:
            return None
        m = b[pos + 1]
        seg = int.from_bytes(b[pos + 2:pos + 4], "big")
        body = b[pos + 4:pos + 2 + seg]
        if seg < 2 or pos + 2 + seg > n:
            return None
        pos += 2 + seg
        if m in (0xC0, 0xC1):                           # baseline / extended sequential, Huffman
            if sof is not None or len(body) < 6:
                return None
            prec, h, w, nf = body[0], int.from_bytes(body[1:3], "big"), \
                int.from_bytes(body[3:5], "big"), body[5]
            if prec != 8 or h == 0 or w == 0 or nf not in (1, 3) or len(body) != 6 + 3 * nf:
                return None
            comps = []
            for i in range(nf):
                cid, hv, tq = body[6 + 3 * i:9 + 3 * i]
                if not (1 <= hv >> 4 <= 4 and 1 <= hv & 15 <= 4) or tq > 3:
                    return None
                comps.append([cid, hv >> 4, hv & 15, tq, 0, 0])
            if nf == 3:
                if [c[0] for c in comps] == [82, 71, 66]:          # 'R', 'G', 'B': no YCbCr
                    return None
                if (comps[1][1:3], comps[2][1:3]) != ([1, 1], [1, 1]) or \
                        tuple(comps[0][1:3]) not in ((1, 1), (2, 1), (2, 2)):
                    return None
            sof = (w, h, comps)
        elif 0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return None                                 # progressive, lossless, arithmetic
        elif m == 0xCC:
            return None
        elif m == 0xDB:                                 # DQT
            o = 0
            while o < len(body):
                pq, tq = body[o] >> 4, body[o] & 15
                size = 64 * (pq + 1)
                if pq > 1 or tq > 3 or o + 1 + size > len(body):
                    return None
                vals = np.frombuffer(body[o + 1:o + 1 + size], dtype=">u2" if pq else np.uint8)
                if vals.max() > MAX_QUANT:
                    return None
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = vals
                qt[tq] = t
                o += 1 + size
        elif m == 0xC4:                                 # DHT
            o = 0
            while o < len(body):
                if o + 17 > len(body):
                    return None
                tc, th = body[o] >> 4, body[o] & 15
                bits = list(body[o + 1:o + 17])
                total = sum(bits)
                if tc > 1 or th > 3 or total > 256 or o + 17 + total > len(body):
                    return None
                vals = bytes(body[o + 17:o + 17 + total])
                if not _canonical_ok(bits):
                    return None
                (ac if tc else dc)[th] = (bits, vals)
                o += 17 + total
        elif m == 0xDD:                                 # DRI
            if len(body) != 2:
                return None
            restart = int.from_bytes(body, "big")
        elif m == 0xE1:
            if body[:6] == b"Exif\0\0":
                if exif_seen:
                    return None
                exif_seen = True
                orientation = _exif_orientation(body[6:])
                if orientation is None:
                    return None
            elif body.startswith(b"http://ns.adobe.com/xap/"):
                return None                             # Pillow also reads XMP orientation
        elif m == 0xEE:
            if body[:5] == b"Adobe":
                return None                             # Adobe colour transform: Pillow's
        elif m == 0xDA:                                 # SOS
            if sof is None or len(body) < 1:
                return None
            w, h, comps = sof
            ns = body[0]
            if ns != len(comps) or len(body) != 4 + 2 * ns:
                return None
            for i in range(ns):
                cid, t = body[1 + 2 * i], body[2 + 2 * i]
                if cid != comps[i][0]:
                    return None
                comps[i][4], comps[i][5] = t >> 4, t & 15
                if t >> 4 > 3 or t & 15 > 3 or dc[t >> 4] is None or ac[t & 15] is None \
                        or qt[comps[i][3]] is None:
                    return None
                if max(dc[t >> 4][1], default=0) > 15:
                    return None                         # libjpeg: a bad DC table
            ss, se, ahl = body[1 + 2 * ns:4 + 2 * ns]
            if ss != 0 or se != 63 or ahl != 0:
                return None
            end = _MARKER_END.search(b, pos)
            if end is None or b[end.start() + 1] != 0xD9:
                return None                             # truncated, a second scan, DNL, ...
            hdr = Header()
            hdr.width, hdr.height = w, h
            hdr.comps = [tuple(c) for c in comps]
            hdr.qt = [q for q in qt]
            hdr.dc, hdr.ac = list(dc), list(ac)
            hdr.restart, hdr.orientation = restart, orientation
            hdr.data_start, hdr.data_end = pos, end.start()
            return hdr
        elif m in (0xD8, 0xD9) or 0xD0 <= m <= 0xD7 or m == 0xDC or m == 0x01:
            return None                                 # out of place, DNL, TEM
        # APPn, COM and the rest: skipped


def _canonical_ok(bits):
    """The code lengths describe a prefix code whose all-ones word stays unused."""
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > (1 << length) - (1 if length == 16 else 0):
            return False
        code <<= 1
    return True


def huff_codes(bits, vals):
    """Canonical code assignment (T.81 C.1 / C.2): [(length, code, symbol)]."""
    out, code, k = [], 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out.append((length, code, vals[k]))
            code += 1
            k += 1
        code <<= 1
    return out


def huff_table(bits, vals):
    """The kernel's lookup table of one Huffman table (HUFF_BYTES): fast[512] = (length << 8) |
    symbol for every 9-bit prefix that holds a whole code of at most 9 bits, else 0;
    maxcode[l] = the largest code of length l (-1: none); valoff[l] = index in vals of the
    first code of length l minus that code; vals padded to 256."""
    fast = np.zeros(512, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    k = 0
    for length, code, sym in huff_codes(bits, vals):
        if length <= 9:
            lo = code << (9 - length)
            fast[lo:lo + (1 << (9 - length))] = (length << 8) | sym
    code = 0
    for length in range(1, 17):
        cnt = bits[length - 1]
        if cnt:
            valoff[length] = k - code
            maxcode[length] = code + cnt - 1
        k += cnt
        code = (code + cnt) << 1
    v = np.zeros(256, np.uint8)
    v[:len(vals)] = np.frombuffer(bytes(vals), np.uint8)
    return fast.tobytes() + maxcode.tobytes() + valoff.tobytes() + v.tobytes()


def _tables(hdr):
    parts = []
    empty = bytes(HUFF_BYTES)
    for t in hdr.dc + hdr.ac:
        parts.append(huff_table(*t) if t is not None else empty)
    for q in hdr.qt:
        parts.append((q if q is not None else np.zeros(64, np.int32)).astype(np.uint16).tobytes())
    out = b"".join(parts)
    assert len(out) == TAB_BYTES
    return out


def _align(x, a=256):
    return (x + a - 1) // a * a


def _image_cost(hdr):
    """(packed bytes, work bytes) one image adds to a batch, as ``pack`` lays it out (the work
    includes its share of the per-batch arrays; each of those arrays' 256-byte rounding is left
    to the batch's slack)."""
    mx, my, bpm = hdr.mcus
    data_len = hdr.data_end - hdr.data_start
    nint = 1 if hdr.restart == 0 else -(-mx * my // hdr.restart)
    chunks = max(1, -(-data_len // CHUNK))
    subs = data_len * 8 // SUBSEQ + nint + 1
    blocks = mx * my * bpm
    packed = TAB_BYTES + _align(data_len, 16)
    work = _align(data_len + 16)
    for _, h, v, *_ in hdr.comps:
        ch, cv = (h, v) if len(hdr.comps) == 3 else (1, 1)
        work += _align(64 * mx * ch * my * cv)
    work += 16 * chunks + 4 + 16 * nint + 36 * subs + 128 * blocks
    return packed, work


_BATCH_SLACK_WORK = 16 * 256        # the rounding of the 14 per-batch work arrays, and spare


def plan_batches(headers, max_packed=BATCH_PACKED, max_work=BATCH_WORK,
                 max_data=MAX_IMAGE_DATA):
    """Split in-scope images into native calls: (batches, rejected).  ``batches`` are lists of
    indices into ``headers``, in order, each within ``max_packed`` packed bytes and ``max_work``
    scratch bytes; ``rejected`` are the images that fit no batch (entropy data over ``max_data``
    bytes, or over a budget alone) - they go to Pillow."""
    if not 0 < max_packed <= MAX_PACKED or max_data > MAX_IMAGE_DATA:
        raise ValueError("batch budget beyond the native limits")
    batches, rejected, cur = [], [], []
    cur_packed = cur_work = 0

    def total(n, packed, work):
        return _align((n + 1) * JD_FIELDS * 8) + packed, work + _BATCH_SLACK_WORK

    for i, hdr in enumerate(headers):
        p, w = _image_cost(hdr)
        alone = total(1, p, w)
        if hdr.data_end - hdr.data_start > max_data or alone[0] > max_packed or \
                alone[1] > max_work:
            rejected.append(i)
            continue
        grown = total(len(cur) + 1, cur_packed + p, cur_work + w)
        if cur and (grown[0] > max_packed or grown[1] > max_work):
            batches.append(cur)
            cur, cur_packed, cur_work = [], 0, 0
        cur.append(i)
        cur_packed += p
        cur_work += w
    if cur:
        batches.append(cur)
    return batches, rejected


def pack(headers, blobs):
    """The batch layout: (desc int64 [n + 1][JD_FIELDS], packed uint8 bytes, work bytes, out
    bytes).  ``desc`` is also the head of ``packed``; output pointers are offsets into one
    output buffer (JD_OUT_OFF)."""
    n = len(headers)
    desc = np.zeros((n + 1, JD_FIELDS), np.int64)
    off = _align(desc.nbytes)
    chunks = ints = subs = blocks = pixels = out = 0
    work = 0
    layout = []
    for i, (hdr, blob) in enumerate(zip(headers, blobs)):
        d = desc[i]
        mx, my, bpm = hdr.mcus
        nmcu = mx * my
        data_len = hdr.data_end - hdr.data_start
        nint = 1 if hdr.restart == 0 else -(-nmcu // hdr.restart)
        d[JD_W], d[JD_H], d[JD_NC] = hdr.width, hdr.height, len(hdr.comps)
        d[JD_HMAX], d[JD_VMAX] = (hdr.hmax, hdr.vmax) if len(hdr.comps) == 3 else (1, 1)
        d[JD_MCUX], d[JD_MCUY], d[JD_BPM] = mx, my, bpm
        d[JD_RI], d[JD_NINT], d[JD_ORIENT] = hdr.restart, nint, hdr.orientation
        d[JD_TAB_OFF] = off
        off = _align(off + TAB_BYTES, 16)
        d[JD_DATA_OFF], d[JD_DATA_LEN] = off, data_len
        layout.append((off, hdr.data_start, hdr.data_end))
        off = _align(off + data_len, 16)
        d[JD_CHUNK0], d[JD_INT0], d[JD_SUB0] = chunks, ints, subs
        d[JD_BLK0], d[JD_PIX0], d[JD_OUT_OFF] = blocks, pixels, out
        chunks += max(1, -(-data_len // CHUNK))
        ints += nint
        subs += data_len * 8 // SUBSEQ + nint + 1
        blocks += nmcu * bpm
        pixels += hdr.width * hdr.height
        out += _align(hdr.width * hdr.height * 3)
        d[JD_DST_OFF] = work
        work = _align(work + data_len + 16)
        comp_u, samp, tabsel = 0, 0, 0
        u = 0
        for c, (_, h, v, tq, td, ta) in enumerate(hdr.comps):
            ch, cv = (h, v) if len(hdr.comps) == 3 else (1, 1)
            for _ in range(ch * cv):
                comp_u |= c << (2 * u)
                u += 1
            samp |= (ch | cv << 4) << (8 * c)
            tabsel |= (td | ta << 2 | tq << 4) << (8 * c)
            bw = mx * ch
            bh = my * cv
            d[JD_PITCH0 + c] = 8 * bw
            d[JD_PLANE0 + c] = work
            work = _align(work + 64 * bw * bh)
        d[JD_COMP_U], d[JD_SAMP], d[JD_TABSEL] = comp_u, samp, tabsel
    bt = desc[n]
    bt[JB_N], bt[JB_CHUNKS], bt[JB_INTS], bt[JB_SUBS] = n, chunks, ints, subs
    bt[JB_BLOCKS], bt[JB_PIXELS], bt[JB_OUT_BYTES] = blocks, pixels, out
    for field, size in ((JB_W_KEPT, 4 * chunks), (JB_W_RST, 4 * chunks), (JB_W_KEPTX, 4 * chunks),
                        (JB_W_RSTX, 4 * chunks), (JB_W_DSTLEN, 4 * max(n, 1)),
                        (JB_W_ISTART, 4 * ints), (JB_W_IEND, 4 * ints), (JB_W_INSUB, 4 * ints),
                        (JB_W_ISUBX, 4 * ints), (JB_W_STATE0, 16 * subs),
                        (JB_W_STATE1, 16 * subs), (JB_W_CNTX, 4 * subs), (JB_W_FLAG, 16),
                        (JB_W_COEF, 128 * blocks)):
        bt[field] = work
        work = _align(work + size)
    bt[JB_WORK_BYTES], bt[JB_PACKED_BYTES] = work, off
    return desc, layout, off


def fill_packed(buf, desc, layout, headers, blobs):
    """Write the batch into ``buf`` (a writable uint8 array of at least packed bytes)."""
    buf[:desc.nbytes] = desc.view(np.uint8).reshape(-1)
    for i, (hdr, blob, (off, a, b)) in enumerate(zip(headers, blobs, layout)):
        t = int(desc[i, JD_TAB_OFF])
        buf[t:t + TAB_BYTES] = np.frombuffer(_tables(hdr), np.uint8)
        buf[off:off + (b - a)] = np.frombuffer(blob, np.uint8, count=b - a, offset=a)


def decode_device(blobs, eng=None, want_coefs=False, _headers=None):
    """One uint8 BGR device tensor [h][w][3] per blob (bytes of an in-scope JPEG), EXIF
    orientation applied.  The batch is packed into one pinned buffer, uploaded once and decoded
    in one native call.  Raises ValueError for a blob ``parse`` rejects.  With ``want_coefs``
    also returns each image's coefficients (int16 [blocks][64], natural order, DC prediction
    applied, in MCU block order)."""
    import torch
    eng = _lib._engine(eng)
    headers = _headers or [parse(b) for b in blobs]
    for i, h in enumerate(headers):
        if h is None:
            raise ValueError(f"blob {i} is not a baseline JPEG the device decodes")
    if not headers:
        return ([], []) if want_coefs else []
    desc, layout, packed_bytes = pack(headers, blobs)
    if packed_bytes > MAX_PACKED or any(h.data_end - h.data_start > MAX_IMAGE_DATA
                                        for h in headers):
        raise ValueError(f"a batch of {packed_bytes} packed bytes is beyond pano_jpeg_decode's "
                         "limits: split it (read_images does)")
    host = torch.empty(packed_bytes, dtype=torch.uint8, pin_memory=True)
    fill_packed(host.numpy(), desc, layout, headers, blobs)
    dev = torch.device(eng.device)
    packed = host.to(dev, non_blocking=True)
    bt = desc[len(headers)]
    work = torch.empty(int(bt[JB_WORK_BYTES]), dtype=torch.uint8, device=dev)
    out = torch.empty(max(int(bt[JB_OUT_BYTES]), 1), dtype=torch.uint8, device=dev)
    desc_c = np.ascontiguousarray(desc)
    eng.call("pano_jpeg_decode", desc_c, len(headers), packed, packed_bytes, work, work.numel(),
             out, out.numel())
    frames = []
    for i, h in enumerate(headers):
        oh, ow = h.out_shape
        o = int(desc[i, JD_OUT_OFF])
        frames.append(out[o:o + oh * ow * 3].view(oh, ow, 3))
    # (the pinned staging buffer: torch's host allocator keeps it until the copy has run)
    if not want_coefs:
        return frames
    coefs = []
    base = int(bt[JB_W_COEF])
    for i, h in enumerate(headers):
        b0 = int(desc[i, JD_BLK0])
        nb = int(desc[i + 1, JD_BLK0]) if i + 1 < len(headers) else int(bt[JB_BLOCKS])
        coefs.append(work[base + 128 * b0:base + 128 * nb].view(torch.int16).view(-1, 64))
    return frames, coefs


def _pillow_read(path):
    """The Pillow path of ``stitcher.ingest`` (what cv2.imread returns: uint8 BGR)."""
    from PIL import Image as PilImage
    from PIL import ImageOps
    im = ImageOps.exif_transpose(PilImage.open(path))
    if im.mode in ("I;16", "I;16B", "I;16L", "I"):
        im = PilImage.fromarray((np.asarray(im).astype(np.uint32) >> 8).astype(np.uint8))
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def read_images(paths, eng=None, max_packed=BATCH_PACKED, max_work=BATCH_WORK,
                max_data=MAX_IMAGE_DATA):
    """Every file of ``paths`` as a uint8 BGR [h][w][3] device tensor, in order, and the path
    each took: "device" (in-scope JPEGs, decoded by ``decode_device`` in batches that
    ``plan_batches`` cuts to the budgets) or "pillow" (everything else, and a JPEG that fits no
    batch, exactly as before)."""
    import torch
    eng = _lib._engine(eng)
    blobs, headers = [], []
    for p in paths:
        with open(p, "rb") as fid:
            blob = fid.read()
        blobs.append(blob)
        headers.append(parse(blob))
    in_scope = [i for i, h in enumerate(headers) if h is not None]
    batches, _ = plan_batches([headers[i] for i in in_scope], max_packed, max_work, max_data)
    frames = [None] * len(paths)
    route = ["pillow"] * len(paths)
    for batch in batches:
        idx = [in_scope[k] for k in batch]
        decoded = decode_device([blobs[i] for i in idx], eng, _headers=[headers[i] for i in idx])
        for i, f in zip(idx, decoded):
            frames[i], route[i] = f, "device"
    for i, r in enumerate(route):
        if r == "pillow":
            frames[i] = torch.from_numpy(_pillow_read(paths[i])).to(eng.device)
    return frames, route


# ---- encode (``pano_jpeg_encode``, ``pano_jpeg_encode_batch``, csrc/jpeg_enc.hip) -------------
# Baseline, 8-bit, YCbCr from RGB, one interleaved scan, no restart markers, the Annex K tables:
# what Pillow's ``Image.save(f, "JPEG")`` writes (libjpeg-turbo's defaults), byte for byte.

# ITU-T T.81 Annex K.1: the example quantisation tables, natural order
STD_LUMA_QT = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int32)
STD_CHROMA_QT = np.full(64, 99, np.int32)
STD_CHROMA_QT.reshape(8, 8)[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99],
                                       [47, 66, 99, 99]]

# ITU-T T.81 Annex K.3: the example Huffman tables, (BITS, HUFFVAL)
STD_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], bytes(range(12)))
STD_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], bytes(range(12)))
STD_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], bytes([
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61,
    0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52,
    0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25,
    0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64,
    0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3,
    0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8,
    0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]))
STD_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], bytes([
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61,
    0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33,
    0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18,
    0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63,
    0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA,
    0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7,
    0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]))
# libjpeg's JPEG_MAX_DIMENSION: a larger side goes to Pillow (which then refuses it, as today)
MAX_ENCODE_SIDE = _lib.JPEG_MAX_SIDE
# Pillow's ``subsampling`` values -> luma (h, v) sampling; the chroma is 1x1
SUBSAMPLING = {-1: (2, 2), 2: (2, 2), 1: (2, 1), 0: (1, 1)}
# the extensions Pillow saves as JPEG (``Image.registered_extensions()``; ".jif" is not one)
JPEG_EXTENSIONS = (".jpg", ".jpeg", ".jpe", ".jfif")


def quant_tables(quality=75):
    """libjpeg's ``jpeg_set_quality(quality, force_baseline=TRUE)``: the Annex K tables scaled
    by ``jpeg_quality_scaling`` and clamped to 1..255; int32 [2][64], natural order."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    out = []
    for base in (STD_LUMA_QT, STD_CHROMA_QT):
        out.append(np.clip((base * scale + 50) // 100, 1, 255))
    return np.stack(out).astype(np.int32)


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def encode_header(width, height, quality=75, subsampling=-1):
    """Everything before the entropy-coded data, with Pillow's marker sequence of a default
    save: SOI, APP0 JFIF 1.01 (no units, 1:1), DQT luma, DQT chroma, SOF0, DHT DC0 / AC0 /
    DC1 / AC1, SOS."""
    qt = quant_tables(quality)
    h, v = SUBSAMPLING[subsampling]
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for t in (0, 1):
        out.append(_segment(0xDB, bytes([t]) + qt[t][ZIGZAG].astype(np.uint8).tobytes()))
    out.append(_segment(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big")
                        + bytes([3, 1, h << 4 | v, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, (bits, vals) in ((0x00, STD_DC_LUMA), (0x10, STD_AC_LUMA),
                                (0x01, STD_DC_CHROMA), (0x11, STD_AC_CHROMA)):
        out.append(_segment(0xC4, bytes([tc_th] + bits) + vals))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


def encodable(img, quality=75, subsampling=-1):
    """Whether ``encode_device`` covers the image and the settings (else Pillow does)."""
    shape = tuple(img.shape)
    return (_lib.is_rgb_u8(img)
            and 1 <= shape[0] <= MAX_ENCODE_SIDE and 1 <= shape[1] <= MAX_ENCODE_SIDE
            and isinstance(quality, (int, np.integer)) and 1 <= quality <= 100
            and subsampling in SUBSAMPLING)


def _encode_setup(images, quality, subsampling, order, eng, numbered):
    """What both encodes do around their native call.  Raises their ValueErrors (``numbered``:
    "image i: " in front); None for no images, before an engine is needed.  Else the engine, the
    calls' flags, subsampling and quantiser table, ``scratch(nbytes)`` (a fresh device tensor, the
    calls' arguments for it) and ``to_file(h, w, address, nbytes)`` (header, stream, EOI)."""
    import torch
    if order not in ("bgr", "rgb"):
        raise ValueError(f"order {order!r}: 'bgr' or 'rgb'")
    for i, img in enumerate(images):
        if not hasattr(img, "shape") or not encodable(img, quality, subsampling):
            raise ValueError(f"image {i}: " * numbered + f"{tuple(getattr(img, 'shape', ()))} "
                             f"{getattr(img, 'dtype', type(img))} at quality {quality}, "
                             f"subsampling {subsampling}: not a case the device encodes")
    if not images:
        return None
    eng = _lib._engine(eng)
    qt = np.ascontiguousarray(quant_tables(quality).astype(np.uint8))
    settings = (_lib.JPEG_BGR if order == "bgr" else 0, 2 if subsampling == -1 else subsampling, qt)

    def scratch(nbytes):
        work = torch.empty(int(nbytes), dtype=torch.uint8, device=torch.device(eng.device))
        return work, (work, int(nbytes))

    def to_file(h, w, address, nbytes):
        return encode_header(w, h, quality, subsampling) + C.string_at(address, nbytes) + b"\xff\xd9"

    return eng, settings, scratch, to_file


def encode_device(img, quality=75, subsampling=-1, order="bgr", eng=None, want_coefs=False):
    """The JPEG file of a uint8 [h][w][3] image (a device tensor, or a host array that is
    uploaded), byte for byte what ``Image.fromarray(rgb).save(f, "JPEG", quality=quality,
    subsampling=subsampling)`` writes.  ``order`` is the channel order of ``img``, "bgr" or
    "rgb".  Any row pitch works as long as the pixels of a row are contiguous (a crop view of a
    mosaic needs no copy).  The quantised blocks are coded by ``pano_jpeg_encode`` in one call
    that waits on the stream twice and downloads the stream; not capturable.  With
    ``want_coefs`` also returns the quantised blocks (int16 [blocks][64] device tensor, natural
    order, DC not differenced, MCU order).  Raises ValueError for what ``encodable`` rejects."""
    import torch
    eng, settings, scratch, to_file = _encode_setup([img], quality, subsampling, order, eng, False)
    img = _lib.rgb_on_device(img, eng)
    h, w = int(img.shape[0]), int(img.shape[1])
    work, work_args = scratch(eng.lib.pano_jpeg_encode_work_bytes(h, w, settings[1]))
    stream, nbytes = C.c_void_p(), C.c_int64()
    eng.call("pano_jpeg_encode", img, h, w, img.stride(0), *settings, *work_args, C.byref(stream),
             C.byref(nbytes))
    data = to_file(h, w, stream.value, nbytes.value)
    if not want_coefs:
        return data
    nblocks = encode_blocks(h, w, subsampling)
    zz = work[:128 * nblocks].view(torch.int16).view(nblocks, 64)
    coefs = torch.empty_like(zz)
    coefs[:, torch.from_numpy(ZIGZAG.astype(np.int64)).to(work.device)] = zz
    return data, coefs


def encode_blocks(h, w, subsampling=-1):
    """Blocks of an h x w image's scan (dummy blocks included): MCUs x blocks per MCU."""
    hm, vm = SUBSAMPLING[subsampling]
    return -(-w // (8 * hm)) * -(-h // (8 * vm)) * (hm * vm + 2)


def plan_encode_batches(blocks, max_work=BATCH_WORK, work_bytes=None):
    """Split images, given their ``encode_blocks``, in order into native calls: lists of indices,
    each within ``max_work`` scratch bytes (``work_bytes(blocks, n)``, by default
    ``pano_jpeg_encode_batch_work_bytes``), ``JPEG_BATCH_MAX`` images and
    ``JPEG_BATCH_MAX_BLOCKS`` blocks.  Raises ValueError for an image that fits no call alone."""
    if work_bytes is None:
        native = _lib.lib().pano_jpeg_encode_batch_work_bytes
        work_bytes = lambda b, n: int(native(b, n))       # noqa: E731

    def fits(b, n):
        return n <= _lib.JPEG_BATCH_MAX and b <= _lib.JPEG_BATCH_MAX_BLOCKS \
            and work_bytes(b, n) <= max_work

    batches, cur, cur_blocks = [], [], 0
    for i, b in enumerate(blocks):
        if not fits(b, 1):
            raise ValueError(f"image {i} of {b} blocks fits no batch of {max_work} scratch bytes")
        if cur and not fits(cur_blocks + b, len(cur) + 1):
            batches.append(cur)
            cur, cur_blocks = [], 0
        cur.append(i)
        cur_blocks += b
    if cur:
        batches.append(cur)
    return batches


def encode_batch_device(images, quality=75, subsampling=-1, order="bgr", eng=None,
                        max_work=BATCH_WORK):
    """One JPEG file (``bytes``) per image of ``images``, a list of uint8 [h][w][3] device tensors
    or views of any sizes (a host array is uploaded): each equals ``encode_device`` of that image.
    A crop view whose rows' pixels are contiguous is coded in place.  The list is cut, in order,
    into native calls (``plan_encode_batches``); ``pano_jpeg_encode_batch`` codes a call's images
    together and waits on the stream twice and downloads once, however many they are.  An empty
    list gives [].  Raises ValueError, before anything is queued, for an image ``encodable``
    rejects."""
    images = list(images)
    setup = _encode_setup(images, quality, subsampling, order, eng, True)
    if setup is None:
        return []
    eng, settings, scratch, to_file = setup
    shapes = [(int(img.shape[0]), int(img.shape[1])) for img in images]
    blocks = [encode_blocks(h, w, subsampling) for h, w in shapes]
    files = []
    for batch in plan_encode_batches(blocks, max_work):
        held = []                                       # uploads and copies live until the call ends
        table = (_lib.JpegImage * len(batch))()
        for rec, i in zip(table, batch):
            img = _lib.rgb_on_device(images[i], eng)
            held.append(img)
            rec.img, rec.pitch, (rec.h, rec.w) = img.data_ptr(), img.stride(0), shapes[i]
        total = sum(blocks[i] for i in batch)
        work, work_args = scratch(eng.lib.pano_jpeg_encode_batch_work_bytes(total, len(batch)))
        streams, offsets = C.c_void_p(), C.c_void_p()
        eng.call("pano_jpeg_encode_batch", table, len(batch), *settings, *work_args,
                 C.byref(streams), C.byref(offsets))
        offs = (C.c_int64 * (len(batch) + 1)).from_address(offsets.value)
        for k, i in enumerate(batch):
            files.append(to_file(*shapes[i], streams.value + offs[k], offs[k + 1] - offs[k]))
    return files


def write(path, img, quality=75, subsampling=-1, order="bgr", eng=None):
    """Save a uint8 [h][w][3] image (device tensor or host array, ``order`` "bgr" or "rgb") as
    the JPEG Pillow would write: on the device when ``encodable``, else through Pillow as
    before.  Returns "device" or "pillow"."""
    if encodable(img, quality, subsampling):
        data = encode_device(img, quality, subsampling, order, eng)
        with open(path, "wb") as fid:
            fid.write(data)
        return "device"
    from PIL import Image as PilImage
    a = img.cpu().numpy() if hasattr(img, "cpu") else np.asarray(img)
    if order == "bgr" and a.ndim == 3:
        a = a[..., ::-1]
    PilImage.fromarray(np.ascontiguousarray(a)).save(path, "JPEG", quality=quality,
                                                     subsampling=subsampling)
    return "pillow"
