"""NumPy restatement of the baseline JPEG decode that csrc/jpeg.hip performs, written from
ITU-T T.81 and libjpeg-turbo's documented default decompression (what Pillow uses): Huffman
decode, DC prediction per restart interval, dequantisation, the ISLOW integer IDCT with its
range-limit table, fancy chroma upsampling, fixed-point YCbCr -> RGB and the EXIF orientation.
Slow (a Python loop per symbol): small images only.  The header comes from
``pano360_amd.jpeg.parse``."""
import numpy as np

from pano360_amd import jpeg as J


class _Bits:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def bit(self):
        byte = self.pos >> 3
        b = self.d[byte] if byte < len(self.d) else 0
        self.pos += 1
        return (b >> (7 - ((self.pos - 1) & 7))) & 1

    def get(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v


def destuff(seg):
    """Entropy-coded segment -> [interval bytes]: FF 00 -> FF, split at RSTn, fill bytes gone."""
    out, cur, i = [], bytearray(), 0
    while i < len(seg):
        b = seg[i]
        if b == 0xFF:
            nxt = seg[i + 1] if i + 1 < len(seg) else None
            if nxt == 0x00:
                cur.append(0xFF)
                i += 2
                continue
            if nxt is not None and 0xD0 <= nxt <= 0xD7:
                out.append(bytes(cur))
                cur = bytearray()
                i += 2
                continue
            i += 1                                      # fill byte
            continue
        cur.append(b)
        i += 1
    out.append(bytes(cur))
    return out


def _decoder(bits, vals):
    return {(length, code): sym for length, code, sym in J.huff_codes(bits, vals)}


def _decode(rd, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | rd.bit()
        if (length, code) in table:
            return table[(length, code)]
    raise ValueError("bad Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def block_order(hdr):
    """Per block of the scan, in MCU order: (component, block x, block y)."""
    mx, my, bpm = hdr.mcus
    out = []
    for m in range(mx * my):
        if len(hdr.comps) == 1:
            out.append((0, m % mx, m // mx))
            continue
        for c, comp in enumerate(hdr.comps):
            h, v = comp[1], comp[2]
            for vy in range(v):
                for hx in range(h):
                    out.append((c, (m % mx) * h + hx, (m // mx) * v + vy))
    return out


def coefficients(hdr, blob):
    """int32 [blocks][64], natural order, MCU block order, DC prediction applied."""
    mx, my, bpm = hdr.mcus
    nmcu = mx * my
    order = block_order(hdr)
    comp_of = [c for c, _, _ in order[:bpm]]
    dct = [_decoder(*t) if t is not None else None for t in hdr.dc]
    act = [_decoder(*t) if t is not None else None for t in hdr.ac]
    intervals = destuff(blob[hdr.data_start:hdr.data_end])
    ri = hdr.restart or nmcu
    out = np.zeros((nmcu * bpm, 64), np.int32)
    for m0 in range(0, nmcu, ri):
        rd = _Bits(intervals[m0 // ri])
        pred = [0] * len(hdr.comps)
        for b in range(m0 * bpm, min(m0 + ri, nmcu) * bpm):
            c = comp_of[b % bpm]
            td, ta = hdr.comps[c][4], hdr.comps[c][5]
            s = _decode(rd, dct[td])
            pred[c] += _extend(rd.get(s), s)
            out[b, 0] = pred[c]
            k = 1
            while k < 64:
                rs = _decode(rd, act[ta])
                r, s = rs >> 4, rs & 15
                if s:
                    k += r
                    out[b, J.ZIGZAG[k]] = _extend(rd.get(s), s)
                    k += 1
                elif r == 15:
                    k += 16
                else:
                    break
    return out


# ---- ISLOW IDCT (CONST_BITS 13, PASS1_BITS 2) ------------------------------------------------
F = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299,
         c1847=15137, c1961=16069, c2053=16819, c2562=20995, c3072=25172)


def _idct_1d(x, shift):
    """One pass over axis -1 of int64 [..., 8]; results DESCALEd by `shift`."""
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * F["c0541"]
    tmp2 = z1 + z3 * -F["c1847"]
    tmp3 = z1 + z2 * F["c0765"]
    tmp0 = (x[..., 0] + x[..., 4]) << 13
    tmp1 = (x[..., 0] - x[..., 4]) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    a0, a1, a2, a3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * F["c1175"]
    a0, a1, a2, a3 = a0 * F["c0298"], a1 * F["c2053"], a2 * F["c3072"], a3 * F["c1501"]
    z1, z2 = z1 * -F["c0899"], z2 * -F["c2562"]
    z3, z4 = z3 * -F["c1961"] + z5, z4 * -F["c0390"] + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    r = lambda v: (v + (1 << (shift - 1))) >> shift
    return np.stack([r(t10 + a3), r(t11 + a2), r(t12 + a1), r(t13 + a0),
                     r(t13 - a0), r(t12 - a1), r(t11 - a2), r(t10 - a3)], axis=-1)


def range_limit(v):
    """libjpeg's post-IDCT table: index (v & 1023), i.e. the 10-bit wrap of v, then clamp of
    v + 128 to [0, 255]."""
    w = (v.astype(np.int64) & 1023)
    w = np.where(w >= 512, w - 1024, w)
    return np.clip(w + 128, 0, 255).astype(np.uint8)


def idct_islow(coef, q):
    """int [n][64] natural-order coefficients, q int [64] -> uint8 [n][8][8]."""
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)
    ws = _idct_1d(np.swapaxes(x, 1, 2), 11)            # columns: CONST_BITS - PASS1_BITS
    ws = np.swapaxes(ws, 1, 2)
    out = _idct_1d(ws, 18)                              # rows: CONST_BITS + PASS1_BITS + 3
    return range_limit(out)


def planes(hdr, coef):
    """Component sample planes (padded to whole blocks) from the coefficients."""
    mx, my, bpm = hdr.mcus
    order = block_order(hdr)
    out = []
    for c, comp in enumerate(hdr.comps):
        h, v = (comp[1], comp[2]) if len(hdr.comps) == 3 else (1, 1)
        out.append(np.zeros((my * v * 8, mx * h * 8), np.uint8))
    for c, comp in enumerate(hdr.comps):
        sel = [i for i, (cc, _, _) in enumerate(order) if cc == c]
        pix = idct_islow(coef[sel], hdr.qt[comp[3]])
        for i, b in enumerate(sel):
            _, bx, by = order[b]
            out[c][8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = pix[i]
    return out


def _clampi(i, n):
    return np.clip(i, 0, n - 1)


def upsample(plane, cw, ch, h, v, width, height):
    """Fancy upsampling of one chroma plane (cw x ch real samples) by (hmax/h, vmax/v) = (1|2,
    1|2) to width x height: the triangle filter with edge replication; a plane of at most two
    samples across is replicated instead (libjpeg's narrow-image case)."""
    p = plane[:ch, :cw].astype(np.int32)
    ys, xs = np.arange(height), np.arange(width)
    if (h, v) == (1, 1):
        return p[:height, :width]
    if cw <= 2:
        return p[_clampi(ys // v, ch)][:, _clampi(xs // h, cw)]
    cx = xs // 2
    if v == 1:          # h2v1
        near = p[:height]
        odd = (xs & 1).astype(bool)
        other = near[:, _clampi(np.where(odd, cx + 1, cx - 1), cw)]
        return (3 * near[:, cx] + other + np.where(odd, 2, 1)) >> 2
    cy = ys // 2        # h2v2
    other_row = _clampi(np.where(ys & 1, cy + 1, cy - 1), ch)
    colsum = 3 * p[cy] + p[other_row]                   # [height][cw]
    odd = (xs & 1).astype(bool)
    other = colsum[:, _clampi(np.where(odd, cx + 1, cx - 1), cw)]
    return (3 * colsum[:, cx] + other + np.where(odd, 7, 8)) >> 4


def ycc_to_bgr(y, cb, cr):
    """libjpeg's fixed-point conversion (SCALEBITS 16), BGR order."""
    y, cb, cr = (a.astype(np.int64) for a in (y, cb, cr))
    cb, cr = cb - 128, cr - 128
    half = 1 << 15
    r = y + ((91881 * cr + half) >> 16)
    g = y + ((-22554 * cb + half - 46802 * cr) >> 16)
    b = y + ((116130 * cb + half) >> 16)
    return np.stack([np.clip(b, 0, 255), np.clip(g, 0, 255), np.clip(r, 0, 255)],
                    axis=-1).astype(np.uint8)


def orient(img, o):
    """ImageOps.exif_transpose's transposition for orientation o."""
    if o == 2:
        return img[:, ::-1]
    if o == 3:
        return img[::-1, ::-1]
    if o == 4:
        return img[::-1]
    if o == 5:
        return np.swapaxes(img, 0, 1)
    if o == 6:
        return np.swapaxes(img, 0, 1)[:, ::-1]
    if o == 7:
        return np.swapaxes(img, 0, 1)[::-1, ::-1]
    if o == 8:
        return np.swapaxes(img, 0, 1)[::-1]
    return img


def decode(blob, hdr=None):
    """uint8 BGR [h][w][3] of an in-scope JPEG."""
    hdr = hdr or J.parse(blob)
    assert hdr is not None
    return pixels(hdr, coefficients(hdr, blob))


def pixels(hdr, coef):
    """uint8 BGR [h][w][3] of the coefficients (``coefficients``' layout) of a header."""
    w, h = hdr.width, hdr.height
    pl = planes(hdr, coef)
    if len(hdr.comps) == 1:
        g = pl[0][:h, :w]
        img = np.stack([g, g, g], axis=-1)
    else:
        hm, vm = hdr.hmax, hdr.vmax
        ch = []
        for c in (1, 2):
            hc, vc = hdr.comps[c][1], hdr.comps[c][2]
            cw, chh = -(-w * hc // hm), -(-h * vc // vm)
            ch.append(upsample(pl[c], cw, chh, hm // hc, vm // vc, w, h))
        img = ycc_to_bgr(pl[0][:h, :w], ch[0], ch[1])
    return np.ascontiguousarray(orient(img, hdr.orientation))


# ---- the device's Huffman synchronisation schedule (jpeg_huff_sync_kernel) ---------------------
def _lut(table):
    """16-bit prefix -> (length << 8) | symbol; an invalid code reads as symbol 0 of 1 bit."""
    lut = np.full(1 << 16, 1 << 8, np.int64)
    for length, code, sym in J.huff_codes(*table):
        lo = code << (16 - length)
        lut[lo:lo + (1 << (16 - length))] = (length << 8) | sym
    return lut.tolist()


def sync_rounds(hdr, blob):
    """The rounds ``pano_jpeg_decode`` runs for this image decoded alone (the
    ``jpeg_huff_sync_kernel`` launch count - 1), restated: each interval is cut into
    ``J.SUBSEQ``-bit subsequences; round 0 decodes each from its first bit, the first of an
    interval in the true state and the others guessing (block 0, coefficient 0); round r
    re-decodes a subsequence only when its predecessor's exit (bit, block, coefficient) changed
    in round r - 1; the rounds end with the first that changes no exit, or at the kernel's
    bound.  Decoding runs while the position is before the subsequence's end; an invalid code
    reads as symbol 0 and consumes 1 bit; bytes past the interval read as zero.  A Python loop
    per symbol: for entropy data up to a few hundred KB."""
    mx, my, bpm = hdr.mcus
    order = block_order(hdr)
    comp_of = [c for c, _, _ in order[:bpm]]
    dcl = {t: _lut(hdr.dc[t]) for t in {c[4] for c in hdr.comps}}
    acl = {t: _lut(hdr.ac[t]) for t in {c[5] for c in hdr.comps}}
    dc_u = [dcl[hdr.comps[c][4]] for c in comp_of]
    ac_u = [acl[hdr.comps[c][5]] for c in comp_of]
    data_len = hdr.data_end - hdr.data_start
    bound = data_len * 8 // J.SUBSEQ + 2
    worst = 1
    for data in destuff(blob[hdr.data_start:hdr.data_end]):
        nbits = 8 * len(data)
        padded = data + bytes(8)
        win = [int.from_bytes(padded[i:i + 4], "big") for i in range(len(data) + 4)]

        def run(pos, u, k, stop):
            while pos < stop:
                w = ((win[pos >> 3] << (pos & 7)) >> 16) & 0xFFFF
                f = (dc_u if k == 0 else ac_u)[u][w]
                pos += f >> 8
                sym = f & 255
                s = sym & 15
                if s:
                    pos += s
                if k == 0:
                    k = 1
                elif s:
                    k += (sym >> 4) + 1
                elif sym >> 4 == 15:
                    k += 16
                else:
                    k = 64
                if k >= 64:
                    k = 0
                    u = u + 1 if u + 1 < bpm else 0
            return pos, u, k

        nsub = max(1, -(-nbits // J.SUBSEQ))
        stops = [min((j + 1) * J.SUBSEQ, nbits) for j in range(nsub)]
        exits = [run(j * J.SUBSEQ, 0, 0, stops[j]) for j in range(nsub)]
        changed = [True] * nsub
        rounds = 0
        while True:
            rounds += 1
            nxt, nchanged = list(exits), [False] * nsub
            for j in range(1, nsub):
                if changed[j - 1]:
                    nxt[j] = run(*exits[j - 1], stops[j])
                    nchanged[j] = nxt[j] != exits[j]
            exits, changed = nxt, nchanged
            if not any(changed) or rounds >= bound:
                break
        worst = max(worst, rounds)
    return min(worst, bound)
