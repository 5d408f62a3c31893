"""Synthetic camera sweeps + frames (SURVEY.md §8d recipes).

No reference code: the reference ships no data set generator.  Cameras are
pinholes with hfov 60 deg on a yaw sweep, optionally jittered; frames are
seeded uint8 noise ("A", stress) or a blurred, rescaled version ("B", smooth,
used for the 1e-4 relative-error criterion).
"""
import numpy as np

from .bundle_adj import intrinsics, rotation_to_mat

HFOV_DEG = 60.0


def focal_for(width, hfov_deg=HFOV_DEG):
    return (width / 2.0) / np.tan(np.deg2rad(hfov_deg) / 2.0)


def make_frame(seed, width, height, kind="A"):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (height, width, 3), dtype=np.uint8)
    if kind == "A":
        return img
    if kind != "B":
        raise ValueError(kind)
    # smooth variant: separable box-ish binomial passes (no SciPy needed so the
    # same bytes are produced everywhere), then stretch to the full range
    f = img.astype(np.float64)
    k = np.array([1, 4, 6, 4, 1], dtype=np.float64) / 16.0
    for _ in range(3):
        f = sum(k[i] * np.roll(f, i - 2, axis=0) for i in range(5))
        f = sum(k[i] * np.roll(f, i - 2, axis=1) for i in range(5))
    lo, hi = f.min(), f.max()
    return np.round((f - lo) * (255.0 / (hi - lo))).astype(np.uint8)


def sweep_yaws(n, sweep_deg=None, step_deg=None):
    if step_deg is not None:
        return np.deg2rad(step_deg) * np.arange(n)
    if n == 1:
        return np.zeros(1)
    return np.deg2rad(sweep_deg) * (np.arange(n) / (n - 1) - 0.5)


def make_cameras(n, width, height, sweep_deg=None, step_deg=None,
                 jitter=0.0, seed=0):
    """Returns (rots [n,3,3], intrs [n,3,3]) float64."""
    yaws = sweep_yaws(n, sweep_deg, step_deg)
    rng = np.random.default_rng(seed)
    intr = intrinsics(focal_for(width))
    rots = []
    for yaw in yaws:
        vec = np.array([0.0, yaw, 0.0])
        if jitter:
            vec = vec + rng.normal(0.0, jitter, 3)
        rots.append(rotation_to_mat(vec))
    return np.stack(rots), np.stack([intr.astype(np.float64)] * n)


# named workloads (BASELINE.json configs 2, 3, 5)
CONFIGS = {
    "cfg2": dict(n=8, width=1920, height=1080, sweep_deg=140.0, n_levels=5),
    "cfg3": dict(n=32, width=3840, height=2160, sweep_deg=155.0, n_levels=5),
    "cfg5": dict(n=120, width=7680, height=4320, step_deg=3.0, n_levels=6),
}


def make_scene(n, width, height, sweep_deg=None, step_deg=None, jitter=0.0,
               seed=0, kind="A", n_levels=5):
    rots, intrs = make_cameras(n, width, height, sweep_deg, step_deg,
                               jitter, seed)
    imgs = [make_frame(seed + i, width, height, kind) for i in range(n)]
    return imgs, rots, intrs


def render_rig(pano, rots, intrs, width, height, device):
    """Frames of a rig looking at one equirectangular panorama (uint8 [H][W][3], host): pixel
    (u, v) of camera i looks along R_i^T K_i^-1 (u - w/2, v - h/2, 1) (the reference's
    conventions, bundle_adj.py:28-29) and takes the panorama's bilinear sample at that ray's
    longitude / latitude (longitude wraps).  Returns uint8 [height][width][3] tensors on
    ``device`` (torch, float64 geometry)."""
    import torch
    ph, pw = pano.shape[:2]
    src = torch.from_numpy(np.ascontiguousarray(pano)).to(device).double()
    vv, uu = torch.meshgrid(torch.arange(height, dtype=torch.float64, device=device),
                            torch.arange(width, dtype=torch.float64, device=device), indexing="ij")
    pix = torch.stack([uu - width / 2, vv - height / 2, torch.ones_like(uu)]).reshape(3, -1)
    frames = []
    for rot, intr in zip(rots, intrs):
        ray = torch.from_numpy(rot.T @ np.linalg.inv(intr)).to(device) @ pix
        theta = torch.atan2(ray[0], ray[2])
        phi = torch.atan2(ray[1], torch.sqrt(ray[0] ** 2 + ray[2] ** 2))
        x = (theta + np.pi) / (2 * np.pi) * pw - 0.5
        y = ((phi + np.pi / 2) / np.pi * ph - 0.5).clamp(0, ph - 1)
        x0, y0 = torch.floor(x), torch.floor(y).clamp(max=ph - 2)
        fx, fy = (x - x0)[:, None], (y - y0)[:, None]
        xi0, yi0 = x0.long() % pw, y0.long()
        xi1 = (xi0 + 1) % pw
        top = src[yi0, xi0] * (1 - fx) + src[yi0, xi1] * fx
        bot = src[yi0 + 1, xi0] * (1 - fx) + src[yi0 + 1, xi1] * fx
        img = top * (1 - fy) + bot * fy
        frames.append(torch.round(img).clamp(0, 255).to(torch.uint8).reshape(height, width, 3)
                      .contiguous())
    return frames
