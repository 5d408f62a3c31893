"""NumPy restatement of the baseline JPEG encode that csrc/jpeg_enc.hip performs, written from
ITU-T T.81 and libjpeg-turbo's default compression (what Pillow's ``Image.save(f, "JPEG")``
runs): RGB -> YCbCr in 16-bit fixed point, edge padding, h2v1 / h2v2 downsampling with
alternating bias, the ISLOW integer FDCT, rounded quantisation, dummy blocks at the right and
bottom edges, and Huffman coding with the Annex K tables, byte stuffing and 1-bit padding.
Everything up to the quantised blocks is vectorised; the Huffman coding loops per coefficient in
Python, so the model is for small images.  The header comes from
``pano360_amd.jpeg.encode_header``."""
import numpy as np

from pano360_amd import jpeg as J


def _fix(x):
    return int(x * 65536 + 0.5)


ONE_HALF = 1 << 15
CBCR_OFFSET = 128 << 16


def rgb_to_ycc(rgb):
    """jccolor.c's rgb_ycc_convert: int64 planes Y, Cb, Cr of a uint8 RGB [h][w][3]."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + ONE_HALF) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.5) * b + CBCR_OFFSET + ONE_HALF - 1) >> 16
    cr = (_fix(0.5) * r - _fix(0.41869) * g - _fix(0.08131) * b + CBCR_OFFSET + ONE_HALF - 1) >> 16
    return y, cb, cr


def geometry(width, height, subsampling):
    """Per component (h, v, blocks across of the component, blocks down, MCU blocks across, MCU
    blocks down) and the MCU grid (mx, my)."""
    hm, vm = J.SUBSAMPLING[subsampling]
    mx, my = -(-width // (8 * hm)), -(-height // (8 * vm))
    comps = []
    for h, v in ((hm, vm), (1, 1), (1, 1)):
        cw, ch = -(-width * h // hm), -(-height * v // vm)
        comps.append((h, v, -(-cw // 8), -(-ch // 8), mx * h, my * v))
    return comps, mx, my


def planes(rgb, subsampling):
    """The component sample planes libjpeg's preprocessing hands to the FDCT, each covering the
    MCU grid (mx * h * 8 columns, my * v * 8 rows; samples of dummy blocks are never used)."""
    height, width = rgb.shape[:2]
    comps, mx, my = geometry(width, height, subsampling)
    ycc = rgb_to_ycc(rgb)
    hm, vm = J.SUBSAMPLING[subsampling]
    out = []
    for c, (h, v, wib, hib, bw, bh) in enumerate(comps):
        cols, rows = np.arange(8 * bw), np.arange(8 * bh)
        full = ycc[c]
        if (h, v) == (hm, vm):                      # full size: replicated right and bottom
            out.append(full[np.minimum(rows, height - 1)][:, np.minimum(cols, width - 1)])
            continue
        x0, x1 = np.minimum(2 * cols, width - 1), np.minimum(2 * cols + 1, width - 1)
        if vm == 1:                                 # h2v1, bias 0, 1, 0, 1, ...
            f = full[np.minimum(rows, height - 1)]
            out.append((f[:, x0] + f[:, x1] + (cols & 1)) >> 1)
            continue
        # h2v2, bias 1, 2, 1, 2, ...: rows of pixel pairs (the last pixel row replicated to
        # fill its pair), then the last downsampled row replicated to the iMCU row's end
        r = np.minimum(rows, -(-height // 2) - 1)
        y0, y1 = np.minimum(2 * r, height - 1), np.minimum(2 * r + 1, height - 1)
        a, b = full[y0], full[y1]
        out.append((a[:, x0] + a[:, x1] + b[:, x0] + b[:, x1] + 1 + (cols & 1)) >> 2)
    return out


# ---- ISLOW FDCT (jfdctint.c: CONST_BITS 13, PASS1_BITS 2) -------------------------------------
F = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299,
         c1847=15137, c1961=16069, c2053=16819, c2562=20995, c3072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, even_shift, odd_shift):
    """One pass over axis -1 of int64 [..., 8]: outputs 0 and 4 shifted by ``even_shift`` (left
    when negative), the rest DESCALEd by ``odd_shift``."""
    tmp0, tmp7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    tmp1, tmp6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    tmp2, tmp5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    tmp3, tmp4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    tmp10, tmp13 = tmp0 + tmp3, tmp0 - tmp3
    tmp11, tmp12 = tmp1 + tmp2, tmp1 - tmp2
    out = [None] * 8
    if even_shift < 0:
        out[0], out[4] = (tmp10 + tmp11) << -even_shift, (tmp10 - tmp11) << -even_shift
    else:
        out[0], out[4] = _descale(tmp10 + tmp11, even_shift), _descale(tmp10 - tmp11, even_shift)
    z1 = (tmp12 + tmp13) * F["c0541"]
    out[2] = _descale(z1 + tmp13 * F["c0765"], odd_shift)
    out[6] = _descale(z1 - tmp12 * F["c1847"], odd_shift)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F["c1175"]
    tmp4, tmp5 = tmp4 * F["c0298"], tmp5 * F["c2053"]
    tmp6, tmp7 = tmp6 * F["c3072"], tmp7 * F["c1501"]
    z1, z2 = z1 * -F["c0899"], z2 * -F["c2562"]
    z3, z4 = z3 * -F["c1961"] + z5, z4 * -F["c0390"] + z5
    out[7] = _descale(tmp4 + z1 + z3, odd_shift)
    out[5] = _descale(tmp5 + z2 + z4, odd_shift)
    out[3] = _descale(tmp6 + z2 + z3, odd_shift)
    out[1] = _descale(tmp7 + z1 + z4, odd_shift)
    return np.stack(out, axis=-1)


def fdct_islow(blocks):
    """int [n][8][8] samples -> int64 [n][8][8] coefficients (scaled by 8, as libjpeg's)."""
    d = blocks.astype(np.int64) - 128
    d = _fdct_1d(d, -2, 13 - 2)                                     # rows
    d = np.swapaxes(_fdct_1d(np.swapaxes(d, 1, 2), 2, 13 + 2), 1, 2)   # columns
    return d


def quantize(coef, q):
    """Rounded division by 8 q with the sign applied after: int64 [n][64] natural order."""
    d = 8 * q.astype(np.int64)
    a = np.abs(coef)
    return np.where(coef < 0, -((a + d // 2) // d), (a + d // 2) // d)


def quantized_blocks(rgb, quality=75, subsampling=-1):
    """int32 [blocks][64]: the quantised blocks in natural order, MCU order, DC not differenced,
    dummy blocks as jccoefct.c makes them (AC zero, DC of the block before)."""
    height, width = rgb.shape[:2]
    comps, mx, my = geometry(width, height, subsampling)
    qt = J.quant_tables(quality)
    pl = planes(rgb, subsampling)
    grids = []
    for c, (h, v, wib, hib, bw, bh) in enumerate(comps):
        p = pl[c].reshape(bh, 8, bw, 8).swapaxes(1, 2).reshape(-1, 8, 8)
        coef = fdct_islow(p).reshape(-1, 64)
        grids.append(quantize(coef, qt[min(c, 1)]).reshape(bh, bw, 64))
    out = []
    for m in range(mx * my):
        ux, uy = m % mx, m // mx
        for c, (h, v, wib, hib, bw, bh) in enumerate(comps):
            for yi in range(v):
                for xi in range(h):
                    bx, by = ux * h + xi, uy * v + yi
                    if by < hib and bx < wib:
                        out.append(grids[c][by, bx])
                    else:
                        blk = np.zeros(64, np.int64)
                        blk[0] = out[-1][0]
                        out.append(blk)
    return np.array(out, np.int32).reshape(-1, 64)


def block_components(subsampling):
    """The component of each block of an MCU."""
    h, v = J.SUBSAMPLING[subsampling]
    return [0] * (h * v) + [1, 2]


class _Writer:
    def __init__(self):
        self.bits = []

    def put(self, code, length):
        self.bits.extend((code >> (length - 1 - i)) & 1 for i in range(length))

    def data(self):
        pad = (-len(self.bits)) % 8
        bits = np.array(self.bits + [1] * pad, np.uint8)
        raw = np.packbits(bits).tobytes()
        return raw.replace(b"\xff", b"\xff\x00")


def _enc_table(bits, vals):
    return {sym: (code, length) for length, code, sym in J.huff_codes(bits, vals)}


_DC = [_enc_table(*J.STD_DC_LUMA), _enc_table(*J.STD_DC_CHROMA)]
_AC = [_enc_table(*J.STD_AC_LUMA), _enc_table(*J.STD_AC_CHROMA)]


def _magnitude(v):
    """(size category, the value's bits) of T.81 F.1.2.1."""
    a = abs(int(v))
    n = a.bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def block_bits(blk, pred, t):
    """[(code, length)] of one block (natural order) given the DC predictor."""
    out = []
    n, b = _magnitude(int(blk[0]) - pred)
    out.append(_DC[t][n])
    if n:
        out.append((b, n))
    zz = blk[J.ZIGZAG]
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(_AC[t][0xF0])
            run -= 16
        n, b = _magnitude(v)
        out.append(_AC[t][(run << 4) | n])
        out.append((b, n))
        run = 0
    if run:
        out.append(_AC[t][0x00])
    return out


def entropy_data(blocks, subsampling):
    """The entropy-coded segment of the quantised blocks (``quantized_blocks``' layout)."""
    comp = block_components(subsampling)
    w = _Writer()
    pred = [0, 0, 0]
    for i, blk in enumerate(blocks):
        c = comp[i % len(comp)]
        for code, length in block_bits(blk, pred[c], min(c, 1)):
            w.put(code, length)
        pred[c] = int(blk[0])
    return w.data()


def encode(rgb, quality=75, subsampling=-1):
    """The JPEG file of a uint8 RGB [h][w][3], as ``Image.fromarray(rgb).save(f, "JPEG",
    quality=quality, subsampling=subsampling)`` writes it."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    height, width = rgb.shape[:2]
    blocks = quantized_blocks(rgb, quality, subsampling)
    return (J.encode_header(width, height, quality, subsampling)
            + entropy_data(blocks, subsampling) + b"\xff\xd9")
