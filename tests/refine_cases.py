"""Seeded rigs for the refinement's tests: rings of ``tests/ba_model.synthetic_matches`` whose true
keypoints are pushed through the forward Brown model on both sides, the cameras ``traverse``
makes of them (the model's walk, on the CPU, so host and GPU tests start from the same cameras),
and the forged pair table of the kernel's sums test.  Test helper only."""
import contextlib
import functools
from collections import defaultdict

import numpy as np

import ba_model
import refine_model as rm
from pano360_amd import bundle_adj as ba

RING = dict(n=8, width=1280, height=720, reach=1)       # f ~ 881: k1 = -0.08 moves corners ~40 px
K_TRUE = (-0.08, 0.0)
DELTA = 3.0


def distorted(matches, focal, k):
    """The match dict with every keypoint pushed through the forward model."""
    out = defaultdict(dict)
    for i in matches:
        for j in matches[i]:
            rows, H, score = matches[i][j]
            rows = np.array(rows, np.float64)
            rows[:, 0:2] = rm.distort_pixels(rows[:, 0:2], focal, k)
            rows[:, 3:5] = rm.distort_pixels(rows[:, 3:5], focal, k)
            out[i][j] = (rows, H, score)
    return out


@functools.lru_cache(maxsize=None)
def ring(kind):
    """kind "clean": no noise, no outliers, 100 matches per pair; "noisy": noise 0.5 px, 3 %
    outliers, 200 per pair.  Both k1 = -0.08.  Returns a dict: matches, truth (rotations, focal),
    index and cameras of the model's traverse, and the flat (rows, table) of refine's pairs.
    Cached: the tests share it and leave it unchanged."""
    if kind == "clean":
        matches, (rots, focal) = ba_model.synthetic_matches(5, per_pair=100, noise=0.0,
                                                            outliers=0.0, **RING)
    else:
        matches, (rots, focal) = ba_model.synthetic_matches(6, per_pair=200, noise=0.5,
                                                            outliers=0.03, **RING)
    matches = distorted(matches, focal, K_TRUE)
    index, cams, _ = ba_model.traverse(RING["n"], matches, badjust="incr")
    pairs = rm.pairs_of(matches, index)
    rows, table = rm.table_of(pairs)
    return {"matches": matches, "rots": rots[index], "focal": focal, "index": index,
            "cameras": cams, "pairs": pairs, "rows": rows, "table": table}


def start_of(case):
    """(f, pp, R) of the case's cameras, the principal points folded into the rotations."""
    cams = case["cameras"]
    return rm.centred(np.array([c.intr[0, 0] for c in cams], np.float64),
                      np.array([[c.intr[0, 2], c.intr[1, 2]] for c in cams], np.float64),
                      np.stack([c.rot for c in cams]).astype(np.float64))


@functools.lru_cache(maxsize=None)
def solved(kind, lens_terms):
    """The model's refinement of ``ring(kind)``: refine_model.lm's record."""
    case = ring(kind)
    f, pp, R = start_of(case)
    return rm.lm(f, pp, R, case["rows"], case["table"], lens_terms=lens_terms, delta=DELTA)


class ModelSums:
    """The model's sums in the place of ``bundle_adj._Refiner``, the device's."""

    def __init__(self, pairs, n, huber):
        self.rows, self.table = rm.table_of(pairs)
        self.n, self.huber = n, huber

    def sums(self, f, pp, R, k):
        cams = np.concatenate([f[:, None], pp, R.reshape(self.n, 9)], axis=1)
        return rm.pair_sums(self.rows, self.table, cams, k, self.huber)[0]


@contextlib.contextmanager
def on_model_sums():
    """``bundle_adj.refine``'s own loop on the model's sums: no GPU."""
    device, ba._Refiner = ba._Refiner, ModelSums
    try:
        yield
    finally:
        ba._Refiner = device


def perturbed_movement(seeds=8, noise=1e-12):
    """What tests/test_gpu_refine.py's tolerances come from: the model's loop on the noisy ring
    with lens_terms = 1, rerun ``seeds`` times with relative uniform noise of ``noise`` on every
    per-pair sum (the counts left exact).  Returns (whether every rerun took the unperturbed
    run's decisions, the largest movement of f relative, of k and of a rotation entry)."""
    case, base = ring("noisy"), solved("noisy", 1)
    f, pp, R = start_of(case)
    same, moved = True, np.zeros(3)
    for seed in range(seeds):
        rng = np.random.default_rng(100 + seed)

        def sums(cams, k):
            out = rm.pair_sums(case["rows"], case["table"], cams, k, DELTA)[0]
            factor = 1 + noise * rng.uniform(-1, 1, out.shape)
            factor[:, [67, 69]] = 1
            return out * factor
        run = rm.lm(f, pp, R, case["rows"], case["table"], lens_terms=1, delta=DELTA, sums=sums)
        same &= [h[2] for h in run["history"]] == [h[2] for h in base["history"]]
        moved = np.maximum(moved, [np.max(np.abs(run["f"] / base["f"] - 1)),
                                   np.max(np.abs(run["k"] - base["k"])),
                                   np.max(np.abs(run["R"] - base["R"]))])
    return same, tuple(float(v) for v in moved)


# ------------------------------------------------------------------ the kernel's sums test
SUM_COUNTS = (0, 1, 63, 64, 65, 256, 257, 600)
SUM_K = (-0.08, 0.01)


def _forge_pair(rng, cams, a, b, count, k, span=(0.6, 0.35), noise=2.0):
    """count rows (x_b, y_b, x_a, y_a): points of camera a's image seen by camera b, distorted."""
    f, pp, rots = cams[:, 0], cams[:, 1:3], cams[:, 3:].reshape(-1, 3, 3)
    ua = rng.uniform([-span[0], -span[1]], [span[0], span[1]], (count, 2))
    v = np.c_[ua, np.ones(count)] @ (rots[b] @ rots[a].T).T
    xa = rm.forward(ua, k) * f[a] + pp[a]
    xb = rm.forward(v[:, :2] / v[:, 2:], k) * f[b] + pp[b] + rng.normal(0, noise, (count, 2))
    return np.c_[xb, xa]


def _forged_cameras(rng):
    rots = ba_model.ring_rotations(rng, 24)[:3]                  # 15 degrees apart
    return np.concatenate([880.0 + rng.uniform(-20, 20, (3, 1)), rng.normal(0, 4, (3, 2)),
                           rots.reshape(3, 9)], axis=1)


def forged_sums(seed=31):
    """3 cameras, one pair per count of SUM_COUNTS (the pairs cycle through (1, 0), (2, 1),
    (0, 2) as (a, b)), for k = SUM_K, noise of 2 px so that some residuals lie beyond delta = 3;
    in the pair of 600 one match at rd = 0 of camera b (its principal point) and one behind
    camera b (a point 79 degrees off camera a's axis, on the far side).  NaN rows before, between
    and after the regions.  Returns a dict: rows, table (int32 [8][4]), cams [3][12]."""
    rng = np.random.default_rng(seed)
    cams = _forged_cameras(rng)
    f, pp, rots = cams[:, 0], cams[:, 1:3], cams[:, 3:].reshape(-1, 3, 3)
    cyc = ((1, 0), (2, 1), (0, 2))
    blocks, table, at = [], [], 0
    for p, count in enumerate(SUM_COUNTS):
        a, b = cyc[p % 3]
        m = _forge_pair(rng, cams, a, b, count, SUM_K)
        if count == 600:
            m[7, 0:2] = pp[b]
            far = [np.array([sign * 5.0, 0.0]) for sign in (1, -1)]
            far = [u for u in far if (rots[b] @ rots[a].T @ np.r_[u, 1.0])[2] < 0][0]
            m[11, 2:4] = rm.forward(far, SUM_K) * f[a] + pp[a]
        gap = int(rng.integers(2, 6))
        blocks += [np.full((gap, 4), np.nan), m]
        table.append((a, b, at + gap, count))
        at += gap + count
    blocks.append(np.full((3, 4), np.nan))
    return {"rows": np.ascontiguousarray(np.concatenate(blocks)),
            "table": np.array(table, np.int32), "cams": cams}


HP_K = (-0.4, 0.0)


def forged_hp(seed=32):
    """One pair of 5 matches near the axis (|u| <= 0.2) for k = HP_K, the third observed by camera
    b at rd = 1.2: h'(rd) = 1 - 1.2 rd^2 < 0 at the first Newton step."""
    rng = np.random.default_rng(seed)
    cams = _forged_cameras(rng)
    m = _forge_pair(rng, cams, 1, 0, 5, HP_K, span=(0.2, 0.2))
    m[2, 0:2] = cams[0, 1:3] + cams[0, 0] * np.array([1.2, 0.0])
    return {"rows": m, "table": np.array([(1, 0, 0, 5)], np.int32), "cams": cams}
