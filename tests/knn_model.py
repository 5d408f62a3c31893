"""NumPy model of ``pano_knn2`` (include/pano360.h; csrc/knn.hip), written from the header and
from the order the kernel states for its exact distances, and the inputs of the tests that hold
the kernel to it bit for bit (tests/test_knn_host.py, tests/test_gpu_knn.py).  The product never
imports this file.

The contract: the answer is exact.  A distance is the float32 sum of squared differences in the
one fixed order of ``knn_exact`` - lane l of 64 takes features l and l + 64, ``df = q[k] - t[k]``
rounded to float32, ``acc = fma(df, df, acc)`` from 0, and the 64 lane values are added by the
butterfly of ``wave_sum`` (partners l ^ 32, ^ 16, ... ^ 1, one float32 addition each) - then
``sqrtf``.  The two nearest rows come first, equal distances: lower index first."""
import numpy as np

KNN_KEEP = 4            # csrc/knn.hip: candidates kept per query
KNN_EPS = 4.0e-5        # csrc/knn.hip: bound on a ranked value, relative to |q|^2 + max |t|^2

_F32_HALF_ULP = np.uint64(0x10000000)      # a float64 whose low 29 bits are these is the
_F32_BELOW = np.uint64(0x1FFFFFFF)         # midpoint of two neighbouring normal float32


def fma32(a, b, c):
    """float32 ``fma(a, b, c)``, rounded once.  The float64 product of two float32 is exact;
    TwoSum gives the float64 sum s and what it lost, e; s -> float32 is the second rounding and
    can only go wrong where s sits exactly on the midpoint of two float32 while e != 0: there
    the sign of e decides, not the tie rule."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32),
                                  np.asarray(c, np.float32))
    shape = a.shape
    p = a.astype(np.float64).ravel() * b.astype(np.float64).ravel()
    c = c.astype(np.float64).ravel()
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    # midpoints of normal float32 by their bits; everything in the denormal range is looked at
    cand = (e != 0) & (((s.view(np.uint64) & _F32_BELOW) == _F32_HALF_ULP)
                       | (np.abs(s) < 2.0 ** -125))
    if cand.any():
        sc, ec, rc = s[cand], e[cand], r[cand]
        toward = np.where(sc > rc, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
        other = np.nextafter(rc, toward)
        mid = (rc.astype(np.float64) != sc) & (rc.astype(np.float64) + other.astype(np.float64)
                                               == 2.0 * sc)
        fixed = np.where(ec > 0, np.maximum(rc, other), np.minimum(rc, other))
        r[cand] = np.where(mid, fixed, rc)
    return r.reshape(shape)


def wave_sum32(v):
    """``wave_sum`` (csrc/wave.h) of float32 [..., 64]: lane 0's value.  After the step with
    partner l ^ o only the lanes below o are still needed, and for them l ^ o = l + o."""
    v = np.asarray(v, np.float32)
    assert v.shape[-1] == 64
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def exact_d2(query, train):
    """float32 [nq][nt]: ``knn_exact`` of every query against every train row, on the unscaled
    inputs."""
    q = np.ascontiguousarray(query, np.float32)
    t = np.ascontiguousarray(train, np.float32)
    (nq, d), nt = q.shape, t.shape[0]
    assert t.shape[1] == d and 1 <= d <= 128
    out = np.empty((nq, nt), np.float32)
    step = max(1, (1 << 21) // (nt * 64))                    # 2 M lane values at a time
    for a in range(0, nq, step):
        df = q[a:a + step, None, :] - t[None, :, :]          # float32 subtraction
        acc = np.zeros(df.shape[:2] + (64,), np.float32)
        first = df[..., :64].astype(np.float64)
        acc[..., :first.shape[-1]] = (first * first).astype(np.float32)    # fma(df, df, +0)
        if d > 64:
            acc[..., :d - 64] = fma32(df[..., 64:], df[..., 64:], acc[..., :d - 64])
        out[a:a + step] = wave_sum32(acc)
    return out


def knn2(query, train, d2=None):
    """(idx int32 [nq][2], dist float32 [nq][2]): the first two rows of a stable sort by
    (``exact_d2``, row index), ``dist = sqrt`` in float32 (correctly rounded, as ``sqrtf``)."""
    if d2 is None:
        d2 = exact_d2(query, train)
    order = np.argsort(d2, axis=1, kind="stable")[:, :2]
    return order.astype(np.int32), np.sqrt(np.take_along_axis(d2, order, axis=1))


def sorted_d2(d2, k):
    """The k smallest values of every row of d2, ascending."""
    return np.sort(d2, axis=1)[:, :k]


# ---------------------------------------------------------------------------------- the cases

def _f32(*arrays):
    return tuple(np.ascontiguousarray(a, np.float32) for a in arrays)


SIFT_SEED = 0


def sift_like(nq=700, nt=1333, d=128, seed=SIFT_SEED):
    """Integer-valued rows as OpenCV's SIFT gives them, Poisson(3) clipped to 255: squared
    distances are exact integers and ties come by themselves."""
    rng = np.random.default_rng(seed)
    return _f32(np.minimum(rng.poisson(3.0, (nq, d)), 255), np.minimum(rng.poisson(3.0, (nt, d)), 255))


def uniform_int(nq, nt, d, seed):
    rng = np.random.default_rng(seed)
    return _f32(rng.integers(0, 256, (nq, d)), rng.integers(0, 256, (nt, d)))


def signed_int(nq, nt, d, seed):
    rng = np.random.default_rng(seed)
    return _f32(rng.integers(-127, 128, (nq, d)), rng.integers(-127, 128, (nt, d)))


# Groups of identical train rows.  Row r of a 32-row tile is in half (r >> 2) & 1 of the wave
# that ranks it (knn2_kernel: register q of lane (n, h) holds row (q & 3) + 8 (q >> 2) + 4 h).
PLANTED_NT = 300
PLANTED_GROUPS = (
    (3, 7),                              # 2: one tile, both halves
    (30, 33, 100),                       # 3: three tiles
    (65, 69, 73, 77, 82),                # 5 > KNN_KEEP: one tile, halves 0 1 0 1 0
    (10, 110, 140, 210, 290),            # 5: five tiles
    (192, 196, 200, 204, 209, 213),      # 6: one tile, halves 0 1 0 1 0 1
    (40, 44, 130, 163, 250, 299),        # 6: two in one tile (both halves), the rest elsewhere
)
PLANTED_PER_GROUP = 6                    # queries per group; the first two equal the row itself


def planted(seed=11):
    """(query, train, group of every query or -1).  Train: uniform 0..255 rows, the groups above
    overwritten with one row each.  Queries per group: the row itself twice, then the row with
    1, 2, 3 and 4 features moved by +-1 or +-2 (every copy stays at the same distance, and every
    other row is some 10^5 away in d2); then 40 rows of their own."""
    rng = np.random.default_rng(seed)
    d = 128
    train = rng.integers(0, 256, (PLANTED_NT, d))
    for rows in PLANTED_GROUPS:
        train[list(rows)] = train[rows[-1]]
    query, group = [], []
    for g, rows in enumerate(PLANTED_GROUPS):
        for k in range(PLANTED_PER_GROUP):
            row = train[rows[0]].copy()
            moved = rng.permutation(d)[:max(0, k - 1)]
            row[moved] += rng.choice((-2, -1, 1, 2), len(moved))
            query.append(row)
            group.append(g)
    query += list(rng.integers(0, 256, (40, d)))
    group += [-1] * 40
    order = rng.permutation(len(query))
    query = np.array(query)[order]
    return _f32(query, train) + (np.array(group)[order],)


OFFSET_NQ, OFFSET_NT, OFFSET_BASE = 150, 400, 200


def offset_int(seed=12):
    """Rows of 200 + {0, 1, 2}: every squared distance is an integer of a few hundred under
    norms of 128 * 201^2, so the whole train set ranks inside the proof's slack."""
    rng = np.random.default_rng(seed)
    return _f32(OFFSET_BASE + rng.integers(0, 3, (OFFSET_NQ, 128)),
                OFFSET_BASE + rng.integers(0, 3, (OFFSET_NT, 128)))


def offset_float(seed=13):
    """The same with a fractional part, 200 + [0, 2): now the split-float16 product really errs,
    by more than neighbouring distances differ, and only the rescan can give the exact order."""
    rng = np.random.default_rng(seed)
    return _f32(OFFSET_BASE + 2.0 * rng.random((OFFSET_NQ, 128)),
                OFFSET_BASE + 2.0 * rng.random((OFFSET_NT, 128)))


TAIL_NQ, TAIL_NT, TAIL_FROM = 80, 1030, 1024


def offset_tail(seed=14):
    """Offset rows again (every query is rescanned), with a train set that reaches past the
    4 * 256 = 1024 waves of ``knn2_rescan_kernel``: its rows 1024.. are visited only in the second
    pass of a wave's loop over ``train``, and the nearest rows of the first queries are there.
    Row 1024 = row 1027 = query 0; row 1025 and row 1026 are queries 1 and 2 with one and two
    features moved; row 5 = row 1028 = query 3 with one feature moved (a tie between a row of the
    first pass and one of the second); row 1029 is query 4 with three features moved."""
    rng = np.random.default_rng(seed)
    q = OFFSET_BASE + rng.integers(0, 3, (TAIL_NQ, 128))
    t = OFFSET_BASE + rng.integers(0, 3, (TAIL_NT, 128))

    def moved(row, n):
        row = row.copy()
        at = rng.permutation(128)[:n]
        row[at] = OFFSET_BASE + (row[at] - OFFSET_BASE + 1) % 3
        return row

    t[1024] = t[1027] = q[0]
    t[1025], t[1026] = moved(q[1], 1), moved(q[2], 2)
    t[5] = t[1028] = moved(q[3], 1)
    t[1029] = moved(q[4], 3)
    return _f32(q, t)


def proof_slack(query, train):
    """KNN_EPS * (|q|^2 + max |t|^2) per query in unscaled d2 units (float64): a ranked value may
    be that far from the true one, so the proof of ``knn2_refine_kernel`` cannot succeed for a
    query whose second and KNN_KEEP-th smallest distances are closer than this."""
    q, t = np.asarray(query, np.float64), np.asarray(train, np.float64)
    return KNN_EPS * ((q * q).sum(1) + (t * t).sum(1).max())


def uniform_float(nq, nt, d, seed):
    rng = np.random.default_rng(seed)
    return _f32(rng.random((nq, d)), rng.random((nt, d)))


def unit_float(nq=700, nt=1333, d=128, seed=2, planted_rows=300):
    """Unit-norm RootSIFT-like rows, the first train rows near duplicates of queries."""
    rng = np.random.default_rng(seed)
    a, b = _f32(rng.random((nq, d)), rng.random((nt, d)))
    a, b = np.sqrt(a / a.sum(1, keepdims=True)), np.sqrt(b / b.sum(1, keepdims=True))
    b[:planted_rows] = (a[rng.permutation(nq)[:planted_rows]]
                        + 1e-3 * rng.random((planted_rows, d)).astype(np.float32))
    return _f32(a, b)


def normal_float(nq, nt, d, seed):
    """Signed, zero-mean rows, as MSOP's normalised patches."""
    rng = np.random.default_rng(seed)
    return _f32(rng.standard_normal((nq, d)), rng.standard_normal((nt, d)))
