"""CPU: the median blend's per-pixel routine (``csrc/median.h``: plain C++ over a sampler, the
text the kernels compile) built into a stand-alone host program with the address and
undefined-behaviour sanitizers and run, through the stage sampler, against ``median_model``: the
golden scenes, a pixel count above PANO_MEDIAN_KEEP (the overflow passes) and forged patches."""
import os
import subprocess

import numpy as np
import pytest

import median_model
from conftest import ROOT, SCENES, load_golden, scene_inputs

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __device__
#define __forceinline__ inline
#define __restrict__
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __fdiv_rn(float a, float b) { return a / b; }
#include "median.h"
// in: int32 n, H, W; per patch int32 y0, x0, h, w, float32 [h][w][4], uint8 mask [h][w]
int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    const float tol = (float)atof(argv[2]);
    int hdr[3];
    if (!f || fread(hdr, 4, 3, f) != 3) return 1;
    const int n = hdr[0], H = hdr[1], W = hdr[2];
    std::vector<pano_patch> table(n);
    std::vector<std::vector<float>> planes(n);
    std::vector<std::vector<uint8_t>> masks(n);
    for (int i = 0; i < n; ++i) {
        int r[4];
        if (fread(r, 4, 4, f) != 4) return 1;
        const size_t px = (size_t)r[2] * r[3];
        std::vector<float> rgba(px * 4);
        masks[i].resize(px);
        if (fread(rgba.data(), 4, rgba.size(), f) != rgba.size()) return 1;
        if (fread(masks[i].data(), 1, px, f) != px) return 1;
        planes[i].resize(px * 4);
        for (size_t p = 0; p < px; ++p)
            for (int c = 0; c < 4; ++c) planes[i][c * px + p] = rgba[p * 4 + c];
        memset(&table[i], 0, sizeof(pano_patch));
        table[i].planes = planes[i].data();
        table[i].mask = masks[i].data();
        table[i].y0 = r[0]; table[i].x0 = r[1]; table[i].h = r[2]; table[i].w = r[3];
        table[i].vh = r[2]; table[i].vw = r[3]; table[i].vpitch = r[3];
    }
    fclose(f);
    static uint32_t mem[2 * MED_KEEP][256];
    std::vector<uint8_t> out((size_t)H * W * 3);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const PatchSampler sm = {table.data(), n, x, y};
            median_pixel(sm, mem, (x * 7 + y) & 255, tol, &out[((size_t)y * W + x) * 3]);
        }
    FILE *o = fopen(argv[3], "wb");
    if (!o || fwrite(out.data(), 1, out.size(), o) != out.size()) return 1;
    fclose(o);
    return 0;
}
"""


@pytest.fixture(scope="module")
def run_pixels(tmp_path_factory):
    """(patches, shape, tol) -> the mosaic the routine gives, uint8 [H][W][3]."""
    tmp = tmp_path_factory.mktemp("median_pixel")
    src, exe = str(tmp / "pixels.cpp"), str(tmp / "pixels")
    with open(src, "w") as fid:
        fid.write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "pano360_amd", "csrc"), src, "-o", exe])

    def run(patches, shape, tol):
        with open(str(tmp / "in.bin"), "wb") as fid:
            fid.write(np.array([len(patches), *shape], np.int32).tobytes())
            for warped, mask, irange in patches:
                fid.write(np.array([irange[0].start, irange[1].start, *warped.shape[:2]],
                                   np.int32).tobytes())
                fid.write(np.ascontiguousarray(warped, np.float32).tobytes())
                fid.write(np.ascontiguousarray(mask).astype(np.uint8).tobytes())
        subprocess.check_call([exe, str(tmp / "in.bin"), repr(float(tol)), str(tmp / "out.bin")])
        return np.fromfile(str(tmp / "out.bin"), np.uint8).reshape(*shape, 3)
    return run


@pytest.mark.parametrize("name", SCENES)
def test_routine_on_the_golden_scenes(oracle, run_pixels, name):
    g = load_golden(name)
    imgs, rots, intrs, mr = scene_inputs(g)
    plan, patches, _ = oracle.warp_all(imgs, rots, intrs, False, mr)
    for tol in (0, 0.02, 0.1, 2):
        want, _ = median_model.median_blend(patches, plan.shape, tol)
        assert np.array_equal(run_pixels(patches, plan.shape, tol), want), tol


def test_routine_consumes_more_samples_than_it_keeps_in_passes(oracle, run_pixels):
    from pano360_amd import _lib, synth
    imgs, rots, intrs = synth.make_scene(260, 32, 24, step_deg=1.3, seed=11, kind="A")
    plan, patches, _ = oracle.warp_all(imgs, rots, intrs, False, 1400)
    assert median_model.sample_counts(patches, plan.shape).max() > _lib.MEDIAN_KEEP
    for tol in (0, 0.1, 0.5, 2):
        want, _ = median_model.median_blend(patches, plan.shape, tol)
        assert np.array_equal(run_pixels(patches, plan.shape, tol), want), tol


def test_routine_on_forged_patches(run_pixels):
    """70 overlapping patches of three colour values a channel (tied keys everywhere), alphas
    that are 0, tiny, above 1 and negative, colours of -0, a fifth of the pixels masked."""
    rng = np.random.default_rng(3)
    patches = []
    for i in range(70):
        warped = np.zeros((9, 13, 4), np.float32)
        warped[..., :3] = rng.integers(0, 3, (9, 13, 3)) / np.float32(2)
        warped[..., 3] = rng.choice(np.array([0, 0, 0.25, 0.5, 1.5, -1, 1e-12], np.float32), (9, 13))
        if i % 5 == 0:
            warped[..., :3] = np.float32(-0.0)
        patches.append((warped, rng.random((9, 13)) < 0.2, np.s_[i % 3:i % 3 + 9, i % 4:i % 4 + 13]))
    assert median_model.sample_counts(patches, (12, 17)).max() > 48      # three overflow passes
    for tol in (0, 0.5, 1):
        want, _ = median_model.median_blend(patches, (12, 17), tol)
        assert np.array_equal(run_pixels(patches, (12, 17), tol), want), tol
