"""Photometric alignment of the frames before the stitch, on the device (``pano_photo_stats``,
``pano_photo_apply_u8``, csrc/photo.hip).

Every camera of a rig meters and white-balances on its own, and every short lens darkens towards
its corners - where a frame's corner meets its neighbour's centre, exactly in the overlap.  The
reference's answer is one scalar gain per camera (``equalize_gains``), which cannot remove a
colour cast and knows nothing of the falloff.  Here camera i is taken to record

    I = g[i][c] V(rho) E        log V(rho) = a1 rho + a2 rho^2 + a3 rho^3

in channel c, with ``g`` a gain per camera and channel, ``V`` one radial falloff shared by all
cameras and ``rho`` the squared distance from the image centre over the squared half diagonal.  A
power-law response keeps the model multiplicative, so it is fitted on the 8-bit values as they
are, and it is linear in the log domain: for a sample seen by cameras i and j the residual is
``d_c - (lg[i][c] - lg[j][c]) - sum_k a_k e_k`` with ``d_c`` the difference of the logs and
``e_k = rho_i^k - rho_j^k``.  The device gathers the 25 sums per camera pair the normal equations
need (``stats_device``), the host solves them in float64 (``solve``), and registration errors and
what moved between the frames are handled by Huber reweighting: a first pass with every weight
1, then ``rounds`` passes with the weight ``min(1, tau / max_c |residual_c|)`` under the previous
pass's parameters.  One streaming kernel applies the result (``apply_device``).

The defaults - ``rounds = 2``, ``tau = 0.05`` (a 5 % exposure difference), the range 16 .. 239
outside of which a pixel is taken as clipped, ``prior = 1e-4`` - were chosen by reasoning, not
tuned on photographs.  ``default_step`` thins the sample lattice to 2^18 points of the largest
frame: on rendered rigs a lattice of 1 775 samples recovered the parameters as well as one of
15 294, so the figure has two orders of magnitude of room; it is not tuned either.
The arithmetic is stated in include/pano360.h and, in NumPy, in tests/photo_model.py.  There is no
CPU fallback.  Not covered: a falloff per camera (mixed lenses), an optical axis away from the
image centre, and a response curve other than a power law.
"""
import logging

import numpy as np

from . import _lib

LO, HI = 16, 239
ROUNDS, TAU, PRIOR = 2, 0.05, 1e-4
LATTICE = 1 << 18
SUMS = _lib.PHOTO_SUMS
TABLE = _lib.PHOTO_TABLE
MODES = {"color": 0, "vignette": 2}
# where the sums of a pair lie (include/pano360.h)
_EE = {(0, 0): 4, (0, 1): 5, (0, 2): 6, (1, 1): 7, (1, 2): 8, (2, 2): 9}


class PhotoModel:
    """What ``solve`` returns: ``log_gains`` float64 [n][3] (each channel's mean over the cameras
    is zero), ``alpha`` float64 [3] (the falloff's coefficients, zero beyond ``terms``), ``rms``
    the weighted RMS residual of the fit (in log units) and ``weight`` the sum of the weights."""
    __slots__ = ("log_gains", "alpha", "rms", "weight")

    def __init__(self, log_gains, alpha=(0.0, 0.0, 0.0), rms=0.0, weight=0.0):
        self.log_gains = np.array(log_gains, np.float64).reshape(-1, 3)
        self.alpha = np.array(alpha, np.float64).reshape(3)
        self.rms, self.weight = float(rms), float(weight)

    def __repr__(self):
        return (f"PhotoModel({len(self.log_gains)} cameras, alpha={tuple(self.alpha)}, "
                f"rms={self.rms:.4g})")

    def log_falloff(self, rho):
        """log V at ``rho``."""
        rho = np.asarray(rho, np.float64)
        a1, a2, a3 = self.alpha
        return (a1 * rho + a2 * (rho * rho)) + a3 * ((rho * rho) * rho)


# ------------------------------------------------------------------- the pairs
def _cone(shape, rot, intr):
    """(unit axis, angular radius) of a cone that holds every ray of a frame: the ray of the
    image centre and its largest angle to the rays of the four corners.  The pixels within an
    angle below 90 degrees of a ray are a convex region of the image plane, so the corners
    decide for the rectangle."""
    h, w = int(shape[0]), int(shape[1])
    hom = np.asarray(rot, np.float64).T @ np.linalg.inv(np.asarray(intr, np.float64))
    pts = np.array([[0.0, -w / 2.0, w / 2.0, -w / 2.0, w / 2.0],
                    [0.0, -h / 2.0, -h / 2.0, h / 2.0, h / 2.0],
                    [1.0, 1.0, 1.0, 1.0, 1.0]])
    rays = hom @ pts
    rays /= np.linalg.norm(rays, axis=0, keepdims=True)
    cosines = np.clip(rays[:, 0] @ rays[:, 1:], -1.0, 1.0)
    return rays[:, 0], float(np.arccos(cosines.min()))


def pair_table(shapes, rots, intrs):
    """The camera pairs (i, j, H), i < j, that can overlap: ``H = (K_j R_j)(R_i^T K_i^-1)`` takes
    centred pixel positions of frame i to those of frame j (float64 [3][3]).  A pair is kept when
    the cones around the two frames' rays can share a ray - the angle between the axes is at most
    the sum of the radii (and a margin of 1e-6) -, or when a radius reaches 90 degrees; a pair
    with a sample shares that sample's ray, so none is dropped.  ``shapes``: (h, w) per camera."""
    n = len(shapes)
    if not (len(rots) == len(intrs) == n):
        raise ValueError(f"{n} shapes, {len(rots)} rotations, {len(intrs)} calibrations")
    if n == 0:
        return []
    cones = [_cone(s, r, k) for s, r, k in zip(shapes, rots, intrs)]
    axes = np.stack([c[0] for c in cones])
    radii = np.array([c[1] for c in cones])
    between = np.arccos(np.clip(axes @ axes.T, -1.0, 1.0))
    wide = radii >= np.pi / 2 - 1e-6
    keep = (between <= radii[:, None] + radii[None, :] + 1e-6) | wide[:, None] | wide[None, :]
    projs = [np.asarray(k, np.float64) @ np.asarray(r, np.float64) for r, k in zip(rots, intrs)]
    homs = [np.asarray(r, np.float64).T @ np.linalg.inv(np.asarray(k, np.float64))
            for r, k in zip(rots, intrs)]
    return [(i, j, projs[j] @ homs[i]) for i in range(n) for j in range(i + 1, n) if keep[i, j]]


def default_step(shapes):
    """The smallest lattice step that leaves at most 2^18 lattice points in the largest frame:
    1 below 512 x 512, 6 for 3840 x 2160.  ``shapes``: (h, w) per camera."""
    step = 1
    for shape in shapes:
        h, w = int(shape[0]), int(shape[1])
        while -(-h // step) * -(-w // step) > LATTICE:
            step += 1
    return step


# -------------------------------------------------------------- the statistics
def _check_frame(i, frame):
    shape = tuple(frame.shape)
    if not _lib.is_rgb_u8(frame):
        raise ValueError(f"frame {i}: {frame.dtype} {shape}, not uint8 [h][w][3]")


def _to_device(frames, eng, min_side):
    """Device tensors whose pixels are 3 bytes apart (rows may be further apart than 3 w)."""
    out = []
    for i, frame in enumerate(frames):
        _check_frame(i, frame)
        if min(frame.shape[:2]) < min_side or max(frame.shape[:2]) > _lib.PHOTO_MAX_SIDE:
            raise ValueError(f"frame {i}: {frame.shape[1]} x {frame.shape[0]} (sides {min_side} .. "
                             f"{_lib.PHOTO_MAX_SIDE})")
        out.append(_lib.rgb_on_device(frame, eng))
    return out


def stats_device(frames, rots, intrs, lo=LO, hi=HI, step=1, params=None, tau=np.inf, eng=None,
                 pairs=None):
    """The 25 sums of every overlapping pair, in ONE native call: (pairs, float64 [P][25]) with
    ``pairs`` from ``pair_table`` (or the given list of (i, j, H)).  ``frames``: uint8 [h][w][3]
    host arrays or device tensors of any sizes, sides >= 2.  ``lo, hi``: a sample counts only when
    both cameras' three values lie in that range; ``step``: every step-th pixel of frame i in x
    and y.  ``params`` (a ``PhotoModel``) and ``tau``: the sample weights are
    ``min(1, tau / max_c |residual_c|)`` under those parameters; None: every weight is 1."""
    import torch
    frames = list(frames)
    n = len(frames)
    if not (len(rots) == len(intrs) == n):
        raise ValueError(f"{n} frames, {len(rots)} rotations, {len(intrs)} calibrations")
    step, lo, hi, tau = int(step), int(lo), int(hi), float(tau)
    if step < 1 or step > _lib.PHOTO_MAX_SIDE:
        raise ValueError(f"step {step}: 1 .. {_lib.PHOTO_MAX_SIDE}")
    if not 1 <= lo <= hi <= 255:
        raise ValueError(f"range [{lo}, {hi}]: 1 <= lo <= hi <= 255")
    if not tau > 0:
        raise ValueError(f"tau {tau}: > 0")
    if params is None:
        log_gains, alpha = np.zeros((n, 3)), np.zeros(3)
    else:
        log_gains = np.ascontiguousarray(params.log_gains, np.float64)
        alpha = np.ascontiguousarray(params.alpha, np.float64)
        if log_gains.shape != (n, 3):
            raise ValueError(f"params: log-gains {log_gains.shape} for {n} frames")
        if not (np.isfinite(log_gains).all() and np.isfinite(alpha).all()):
            raise ValueError("params: a parameter is not finite")
    eng = _lib._engine(eng)
    frames = _to_device(frames, eng, 2)
    if pairs is None:
        pairs = pair_table([f.shape[:2] for f in frames], rots, intrs)
    pairs = [(int(i), int(j), np.asarray(H, np.float64).reshape(3, 3)) for i, j, H in pairs]
    for i, j, H in pairs:
        if not (0 <= i < n and 0 <= j < n and i != j):
            raise ValueError(f"pair ({i}, {j}) of {n} frames")
        if not np.isfinite(H).all():
            raise ValueError(f"pair ({i}, {j}): H is not finite")
    if not pairs:
        return pairs, np.zeros((0, SUMS))
    frame_recs = (_lib.PhotoFrame * n)()
    for rec, frame in zip(frame_recs, frames):
        rec.img, rec.pitch = frame.data_ptr(), frame.stride(0)
        rec.w, rec.h = int(frame.shape[1]), int(frame.shape[0])
    pair_recs = (_lib.PhotoPair * len(pairs))()
    for rec, (i, j, H) in zip(pair_recs, pairs):
        rec.H[:] = H.ravel().tolist()
        rec.i, rec.j = i, j
    sums = torch.empty((len(pairs), SUMS), dtype=torch.float64, device=frames[0].device)
    eng.call("pano_photo_stats", frame_recs, n, pair_recs, len(pairs), step, lo, hi, log_gains,
             alpha, tau, sums)
    return pairs, sums.cpu().numpy()


# ------------------------------------------------------------------- the solve
def solve(n, pairs, sums, terms=2, prior=PRIOR):
    """The least-squares parameters of ``n`` cameras from the pairs' sums, on the host in
    float64: 3 n log-gains and ``terms`` (0 .. 3) falloff coefficients by ``np.linalg.solve`` of
    the normal equations, with a ridge of ``prior * sum(w) / n`` on every log-gain (it fixes the
    gauge: only differences of log-gains are observed); afterwards each channel's log-gains have
    their mean subtracted.  ``ValueError`` when the system is singular (a falloff term the samples
    do not determine).  No sample at all: gains of 1, no falloff, and a logged warning."""
    n, terms = int(n), int(terms)
    if n < 1:
        raise ValueError(f"{n} cameras")
    if not 0 <= terms <= 3:
        raise ValueError(f"terms {terms}: 0 .. 3")
    if not prior > 0:
        raise ValueError(f"prior {prior}: > 0")
    sums = np.asarray(sums, np.float64).reshape(-1, SUMS)
    if len(sums) != len(pairs):
        raise ValueError(f"{len(pairs)} pairs, {len(sums)} rows of sums")
    if not np.isfinite(sums).all():
        raise ValueError("a sum is not finite")
    total = float(sums[:, 0].sum())
    if not total > 0:
        logging.warning("Photometric alignment: no camera pair has a usable sample in its overlap; "
                        "gains of 1 and no falloff")
        return PhotoModel(np.zeros((n, 3)))
    size = 3 * n + terms
    A, b = np.zeros((size, size)), np.zeros(size)
    dd = 0.0
    for (i, j, _), S in zip(pairs, sums):
        for c in range(3):
            base = 10 + 5 * c
            ic, jc = 3 * i + c, 3 * j + c
            A[ic, ic] += S[0]
            A[jc, jc] += S[0]
            A[ic, jc] -= S[0]
            A[jc, ic] -= S[0]
            b[ic] += S[base]
            b[jc] -= S[base]
            dd += S[base + 4]
            for k in range(terms):
                A[ic, 3 * n + k] += S[1 + k]
                A[3 * n + k, ic] += S[1 + k]
                A[jc, 3 * n + k] -= S[1 + k]
                A[3 * n + k, jc] -= S[1 + k]
                b[3 * n + k] += S[base + 1 + k]
                for m in range(terms):
                    A[3 * n + k, 3 * n + m] += S[_EE[(min(k, m), max(k, m))]]
    ridge = np.zeros(size)
    ridge[:3 * n] = prior * total / n
    try:
        theta = np.linalg.solve(A + np.diag(ridge), b)
    except np.linalg.LinAlgError as err:
        raise ValueError(f"the normal equations of the photometric fit are singular ({err}): "
                         f"{terms} falloff terms are not determined by these overlaps") from None
    if not np.isfinite(theta).all():
        raise ValueError("the normal equations of the photometric fit are singular")
    rss = dd - 2.0 * theta.dot(b) + theta.dot(A.dot(theta))
    log_gains = theta[:3 * n].reshape(n, 3)
    log_gains = log_gains - log_gains.mean(axis=0, keepdims=True)
    alpha = np.zeros(3)
    alpha[:terms] = theta[3 * n:]
    return PhotoModel(log_gains, alpha, np.sqrt(max(rss, 0.0) / (3 * total)), total)


def estimate_device(frames, rots, intrs, terms=2, rounds=ROUNDS, tau=TAU, lo=LO, hi=HI, step=None,
                    prior=PRIOR, eng=None):
    """The ``PhotoModel`` of a registered rig: a pass with every weight 1, then ``rounds``
    passes reweighted with the Huber threshold ``tau`` under the pass before's parameters; every
    pass is one ``stats_device`` over all pairs and one ``solve``.  ``step`` None:
    ``default_step``.  The frames are uploaded once.  Logs the gains, the falloff at the corner
    and the RMS residual at INFO."""
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError(f"rounds {rounds}: >= 0")
    eng = _lib._engine(eng)
    frames = _to_device(list(frames), eng, 2)
    shapes = [f.shape[:2] for f in frames]
    if step is None:
        step = default_step(shapes)
    pairs = pair_table(shapes, rots, intrs)
    model = None
    for _ in range(rounds + 1):
        _, sums = stats_device(frames, rots, intrs, lo, hi, step, model,
                               np.inf if model is None else tau, eng, pairs)
        model = solve(len(frames), pairs, sums, terms, prior)
        if not model.weight > 0:
            break
    gains = np.exp(model.log_gains)
    for i, g in enumerate(gains):
        logging.info(f"Photometric alignment, camera {i}: gains {g[0]:.4f} {g[1]:.4f} {g[2]:.4f}")
    logging.info(f"Photometric alignment: {len(pairs)} pairs, step {step}, weight "
                 f"{model.weight:.1f}, falloff at the corner "
                 f"{float(np.exp(model.log_falloff(1.0))):.4f}, RMS residual {model.rms:.5f}")
    return model


# -------------------------------------------------------------- the correction
def tables(model):
    """float32 [n][3][1026]: ``T[c][k] = float32(exp(-lg[c] - log V(rho_k)))``, ``rho_k = k /
    1024`` - what a camera's pixels are multiplied with, the kernel interpolating in ``k``."""
    rho = np.arange(TABLE, dtype=np.float64) / 1024.0
    fall = model.log_falloff(rho)
    return np.exp(-model.log_gains[:, :, None] - fall[None, None, :]).astype(np.float32)


def apply_device(frames, model, eng=None):
    """New uint8 device tensors: every frame divided by its camera's gains and the falloff, in
    ONE native call (``pano_photo_apply_u8``: the factor from the camera's table, linear in
    ``1024 rho``, the product rounded and clamped to 255).  ``frames``: uint8 [h][w][3] host
    arrays or device tensors of any sizes, one per camera of ``model``."""
    import torch
    frames = list(frames)
    if len(frames) != len(model.log_gains):
        raise ValueError(f"{len(frames)} frames for a model of {len(model.log_gains)} cameras")
    if not frames:
        return []
    eng = _lib._engine(eng)
    frames = _to_device(frames, eng, 1)
    device = frames[0].device
    table = torch.from_numpy(tables(model)).to(device)
    records = (_lib.PhotoApply * len(frames))()
    outs = []
    for k, (rec, frame) in enumerate(zip(records, frames)):
        out = torch.empty((frame.shape[0], frame.shape[1], 3), dtype=torch.uint8, device=device)
        rec.src, rec.dst, rec.table = frame.data_ptr(), out.data_ptr(), table[k].data_ptr()
        rec.src_pitch, rec.dst_pitch = frame.stride(0), out.stride(0)
        rec.w, rec.h = int(frame.shape[1]), int(frame.shape[0])
        outs.append(out)
    eng.call("pano_photo_apply_u8", records, len(frames))
    # (the kernels are queued on the stream the tensors belong to: `frames` and `table` may go)
    return outs


def correct_regions(regions, terms=2, eng=None):
    """``estimate_device`` on the registered frames ``regions`` (``bundle_adj.Image``: ``img``
    a host uint8 array or a device tensor, ``rot``, ``intr``), then every ``reg.img`` replaced by
    the corrected device tensor.  Returns the ``PhotoModel``."""
    frames = [reg.img for reg in regions]
    rots, intrs = [reg.rot for reg in regions], [reg.intr for reg in regions]
    eng = _lib._engine(eng)
    frames = _to_device(frames, eng, 2)
    model = estimate_device(frames, rots, intrs, terms=terms, eng=eng)
    for reg, frame in zip(regions, apply_device(frames, model, eng)):
        reg.img = frame
    return model


# ------------------------------------------------------------- command line
def add_arguments(parser):
    """``--photometric`` of stitcher.py.  Without the flag the parsed namespace is what it was
    (no ``photometric`` attribute: ``mode_of`` reads it)."""
    import argparse
    parser.add_argument("--photometric", choices=list(MODES), default=argparse.SUPPRESS,
                        help="match the frames' exposure and white balance before the stitch, on "
                             "the device: 'color' fits a gain per camera and channel over all "
                             "overlaps, 'vignette' also the lens's radial falloff (not with "
                             "--equalize).")


def mode_of(args):
    """"color", "vignette" or None: what ``--photometric`` asked for."""
    return getattr(args, "photometric", None)


def check_arguments(parser, args):
    if mode_of(args) is not None and args.equalize:
        parser.error("--photometric and --equalize exclude each other: both set the exposure")
