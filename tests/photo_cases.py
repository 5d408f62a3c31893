"""The forged rigs of tests/test_photo_host.py and tests/test_gpu_photo.py.  Every frame is
``synth.render_rig`` (on the CPU) of one smooth seeded panorama with values in 50 .. 200, then
multiplied by the case's known gains and falloff and rounded: the truth the fit must recover.
Model results are computed once per case and shared read-only."""
import functools

import numpy as np

import photo_model as pm

LO, HI = 16, 239
ALPHA = (-0.45, 0.10, 0.0)

# name -> sizes (w, h) per camera, sweep in degrees, jitter, and what is done to the frames
CASES = {
    "rig5": dict(sizes=[(96, 64)] * 5, sweep=100.0, jitter=0.02, alpha=ALPHA),
    # narrower than a statistics tile, 1.5 tile rows
    "rig3": dict(sizes=[(40, 24)] * 3, sweep=50.0, jitter=0.0, alpha=ALPHA),
    "mixed": dict(sizes=[(96, 64), (48, 40), (96, 64), (48, 40)], sweep=75.0, jitter=0.01,
                  alpha=ALPHA),
    # two cameras 170 degrees apart: no sample
    "apart": dict(sizes=[(96, 64)] * 2, sweep=170.0, jitter=0.0, alpha=ALPHA),
    # a sweep over more than 180 degrees: the far pairs have Z <= 0 everywhere
    "behind": dict(sizes=[(96, 64)] * 6, sweep=200.0, jitter=0.01, alpha=ALPHA),
    # the last frame is all 255: every sample of its pairs is excluded
    "clipped": dict(sizes=[(96, 64)] * 5, sweep=100.0, jitter=0.02, alpha=ALPHA, clip=4),
    # "someone walked through": two rectangles (camera, x0, y0, w, h, colour) painted over.  A
    # Huber weight bounds an outlier's pull at tau instead of removing it, so what is left of the
    # bias is about tau times the outliers' share of a pair's samples: 288 of ~3500 at tau = 0.05
    # is 0.004 at the most, and their unweighted pull (a log difference near 1) is 0.08.
    "walker": dict(sizes=[(96, 64)] * 5, sweep=100.0, jitter=0.02, alpha=ALPHA,
                   paint=[(1, 30, 10, 12, 24, (40, 60, 90)), (3, 50, 20, 10, 20, (190, 170, 60))]),
    "flat": dict(sizes=[(96, 64)] * 5, sweep=100.0, jitter=0.02, alpha=(0.0, 0.0, 0.0)),
}
# the cases whose truth a fit can recover: every camera is tied to the others by samples
RECOVERABLE = ("rig5", "rig3", "mixed", "behind", "walker", "flat")
STEPS = (1, 3)


@functools.lru_cache(maxsize=None)
def panorama():
    """uint8 [256][512][3], smooth, 50 .. 200: a few low harmonics per channel (whole periods
    around the longitude, so the wrap is smooth too)."""
    rng = np.random.default_rng(2024)
    ph, pw = 256, 512
    phi, theta = np.mgrid[0:ph, 0:pw]
    theta = theta * (2 * np.pi / pw)
    phi = phi * (np.pi / ph)
    planes = []
    for _ in range(3):
        f = np.zeros((ph, pw))
        for _ in range(8):
            kx, ky = int(rng.integers(1, 7)), float(rng.uniform(0.5, 5.0))
            f += rng.uniform(0.3, 1.0) * np.cos(kx * theta + rng.uniform(0, 2 * np.pi)) * \
                np.cos(ky * phi + rng.uniform(0, 2 * np.pi))
        planes.append(50.0 + 150.0 * (f - f.min()) / (f.max() - f.min()))
    pano = np.rint(np.stack(planes, axis=-1)).astype(np.uint8)
    pano.setflags(write=False)
    return pano


@functools.lru_cache(maxsize=None)
def cameras(name):
    """(rots [n][3][3], intrs [n][3][3]) of the case."""
    from pano360_amd import bundle_adj, synth
    case = CASES[name]
    n = len(case["sizes"])
    rots, _ = synth.make_cameras(n, 96, 64, sweep_deg=case["sweep"], jitter=case["jitter"], seed=7)
    intrs = np.stack([np.asarray(bundle_adj.intrinsics(synth.focal_for(w)), np.float64)
                      for w, _ in case["sizes"]])
    rots.setflags(write=False)
    intrs.setflags(write=False)
    return rots, intrs


@functools.lru_cache(maxsize=None)
def truth(name):
    """(log-gains [n][3] with each channel's mean zero, alpha [3]): gains within +-20 %."""
    n = len(CASES[name]["sizes"])
    rng = np.random.default_rng(31 + n)
    lg = np.log(rng.uniform(0.8, 1.2, size=(n, 3)))
    lg -= lg.mean(axis=0, keepdims=True)
    lg.setflags(write=False)
    return lg, np.asarray(CASES[name]["alpha"], np.float64)


@functools.lru_cache(maxsize=None)
def clean_frames(name):
    """The rig's frames before gains and falloff (uint8, read-only)."""
    import torch
    from pano360_amd import synth
    rots, intrs = cameras(name)
    out = []
    for (w, h), rot, intr in zip(CASES[name]["sizes"], rots, intrs):
        frame = synth.render_rig(np.array(panorama()), [rot], [intr], w, h,
                                 torch.device("cpu"))[0].numpy()
        frame.setflags(write=False)
        out.append(frame)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def frames(name):
    """The case's frames as the cameras recorded them (uint8, read-only)."""
    case = CASES[name]
    lg, alpha = truth(name)
    out = []
    for k, clean in enumerate(clean_frames(name)):
        h, w = clean.shape[:2]
        factor = np.exp(lg[k][None, None, :] + pm.log_falloff(alpha, pm.rho_grid(w, h))[..., None])
        frame = np.clip(np.rint(clean.astype(np.float64) * factor), 0, 255).astype(np.uint8)
        for cam, x0, y0, pw, ph, colour in case.get("paint", ()):
            if cam == k:
                frame[y0:y0 + ph, x0:x0 + pw] = colour
        if case.get("clip") == k:
            frame[:] = 255
        frame.setflags(write=False)
        out.append(frame)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pairs(name):
    """Every (i, j, H), i < j, by the model's own homography."""
    return tuple(pm.all_pairs(*cameras(name)))


@functools.lru_cache(maxsize=None)
def first_pass(name, step):
    """(sums, scales) of the pass with every weight 1."""
    sums, scale = pm.stats(frames(name), pairs(name), LO, HI, step)
    sums.setflags(write=False)
    scale.setflags(write=False)
    return sums, scale


@functools.lru_cache(maxsize=None)
def first_params(name, step, terms=2):
    """(log_gains, alpha) of the model's solve of the first pass."""
    return pm.solve(len(frames(name)), pairs(name), first_pass(name, step)[0], terms)


@functools.lru_cache(maxsize=None)
def second_pass(name, step):
    """(sums, scales) of a pass reweighted with tau = 0.05 under ``first_params``."""
    lg, alpha = first_params(name, step)
    sums, scale = pm.stats(frames(name), pairs(name), LO, HI, step, lg, alpha, 0.05)
    sums.setflags(write=False)
    scale.setflags(write=False)
    return sums, scale


@functools.lru_cache(maxsize=None)
def estimate(name, rounds=2, step=1, terms=2):
    """The model's own estimate: (log_gains, alpha, first pass's (log_gains, alpha))."""
    return pm.estimate(frames(name), pairs(name), terms, rounds, 0.05, LO, HI, step)


def errors(name, log_gains, alpha):
    """(max |delta log-gain|, max |delta log V| over the frames' pixels) against the truth."""
    lg, true_alpha = truth(name)
    worst = 0.0
    for w, h in set(CASES[name]["sizes"]):
        rho = pm.rho_grid(w, h)
        worst = max(worst, float(np.abs(pm.log_falloff(alpha, rho) - pm.log_falloff(true_alpha, rho)).max()))
    return float(np.abs(np.asarray(log_gains) - lg).max()), worst
