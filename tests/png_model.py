"""NumPy restatement of the device PNG encoder's two rules (csrc/png_enc.hip): the scanline
filters with their per-row choice, and the run tokeniser of the deflate coder."""
import numpy as np

CHUNK = 65536
MAX_MATCH = 258


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def candidates(rgb):
    """The five filtered versions of every row: uint8 [5][h][3 w].  Bytes left of the row and
    the row above row 0 count as 0; Average is (left + up) >> 1; Paeth breaks ties in the order
    left, up, upper left."""
    h, w = rgb.shape[:2]
    x = rgb.reshape(h, 3 * w).astype(np.int64)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]).astype(np.uint8)


def choose(cands):
    """Per row the filter with the smallest sum of |filtered byte as int8|, the first minimum in
    the order 0 .. 4."""
    cost = np.abs(cands.view(np.int8).astype(np.int64)).sum(axis=2)     # [5][h]
    return np.argmin(cost, axis=0)


def scanlines(rgb, choice=None):
    """The PNG scanlines of a uint8 RGB image [h][w][3]: uint8 [h][1 + 3 w], the filter's number
    then the filtered row.  ``choice`` overrides the rule (one filter number per row)."""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    cands = candidates(rgb)
    pick = choose(cands) if choice is None else np.broadcast_to(np.asarray(choice), (h,))
    out = np.empty((h, 1 + 3 * w), np.uint8)
    out[:, 0] = pick
    out[:, 1:] = cands[pick, np.arange(h)]
    return out


def tokens(data, chunk=CHUNK):
    """The deflate coder's tokens, one list per chunk of ``chunk`` bytes (one empty list for no
    data): (position, 0) for a literal, (position, length) for a match at distance 1.  Runs of
    equal bytes are maximal over the whole buffer.  A run's first byte is a literal; the rest of
    it, cut at the chunk borders, is matches of 258 and one of the remainder, or 1 - 2 literals
    when that is below 3.  A run that began before a chunk has no first byte in it: its matches
    there reach the byte before the chunk."""
    d = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1)
    n = len(d)
    start = np.ones(n, bool)
    start[1:] = d[1:] != d[:-1]
    out = []
    for c0 in range(0, max(n, 1), chunk):
        c1 = min(c0 + chunk, n)
        first = start[c0:c1].copy()
        first[:1] = True
        seg = np.flatnonzero(first) + c0
        toks = []
        for a, e in zip(seg.tolist(), seg[1:].tolist() + [c1]):
            p = a
            if start[a]:
                toks.append((a, 0))
                p += 1
            while e - p >= 3:
                length = min(MAX_MATCH, e - p)
                toks.append((p, length))
                p += length
            toks.extend((q, 0) for q in range(p, e))
        out.append(toks)
    return out


def expand(data, toks):
    """The bytes the tokens of ``tokens`` stand for, decoded as a deflate decoder would (a
    literal's value is read from ``data``; a match copies the byte before it)."""
    d = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1)
    out = bytearray()
    for chunk in toks:
        for pos, length in chunk:
            assert pos == len(out)
            if length == 0:
                out.append(int(d[pos]))
            else:
                assert len(out) >= 1
                out.extend(out[-1:] * length)
    return bytes(out)
