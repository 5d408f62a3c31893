"""GPU: ``pano_crop_rect`` (csrc/crop.hip) on the forged masks of tests/crop_cases.py against the
NumPy model of its contract, tests/crop_model.py: the rectangle, the reported area and the whole
``heights`` plane, by integer equality.  The native entry is called directly, since
``engine.crop_rect`` hides ``heights`` and the area.  What the cases depend on is asserted on the
model alone in tests/test_crop_host.py."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crop_cases as cc  # noqa: E402
import crop_model as cm  # noqa: E402

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -1
SENTINEL = -77


@functools.lru_cache(maxsize=None)
def _model(name):
    """(result[0..5], heights) of the model, computed once and read-only."""
    mask = cc.CASES[name]
    (y0, x0, h, w), area = cm.crop_rect(mask)
    hgt = cm.heights(mask)
    hgt.setflags(write=False)
    return (1, y0, x0, h, w, area), hgt


def _native(eng, mask, H=None, W=None, null=(), result_fill=SENTINEL, heights_fill=SENTINEL):
    """pano_crop_rect into prefilled outputs: (status, result, heights, mask afterwards) on the
    host.  The buffers have the sizes of ``mask`` whatever H and W claim."""
    import torch
    from pano360_amd import _lib
    dev = dict(valid=torch.from_numpy(np.array(mask)).to(eng.device),
               heights=torch.full(mask.shape, heights_fill, dtype=torch.int32, device=eng.device),
               result=torch.full((6,), result_fill, dtype=torch.int64, device=eng.device))
    ptr = {key: None if key in null else _lib._ptr(v) for key, v in dev.items()}
    status = eng.lib.pano_crop_rect(eng.ctx(), ptr["valid"], mask.shape[0] if H is None else H,
                                    mask.shape[1] if W is None else W, ptr["heights"],
                                    ptr["result"])
    torch.cuda.synchronize()
    return (status, dev["result"].cpu().numpy(), dev["heights"].cpu().numpy(),
            dev["valid"].cpu().numpy())


def _assert_model(out, name):
    status, result, heights, mask_after = out
    want_result, want_heights = _model(name)
    assert status == OK, name
    assert tuple(int(v) for v in result) == want_result, name
    assert heights.dtype == np.int32 and heights.shape == want_heights.shape
    bad = np.argwhere(heights != want_heights)
    if len(bad):
        i, j = bad[0]
        raise AssertionError(f"{name}: {len(bad)} heights differ, the first at ({i}, {j}): "
                             f"{heights[i, j]}, the model has {want_heights[i, j]}")
    assert np.array_equal(mask_after, cc.CASES[name]), name


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_rectangle_heights_and_area_equal_the_model(eng, name):
    _assert_model(_native(eng, cc.CASES[name]), name)


@pytest.mark.parametrize("shape", cc.EMPTY_SHAPES)
def test_empty_masks(eng, shape):
    import torch
    mask = np.zeros(shape, np.uint8)
    status, result, heights, mask_after = _native(eng, mask)
    assert status == OK
    assert result.tolist() == [0] * 6
    assert not heights.any() and not mask_after.any()
    assert eng.crop_rect(torch.from_numpy(mask).to(eng.device)) is None


@pytest.mark.parametrize("name", sorted(cc.TIES) + sorted(cc.STAIRS))
def test_three_runs_give_the_same_bytes(eng, name):
    """The workgroups raise one cell concurrently and prune by what they read there: the same
    bytes every time, also from a ``result`` of 0xFF bytes - the call sets the cell itself."""
    mask = cc.CASES[name]
    runs = [_native(eng, mask) for _ in range(3)]
    runs.append(_native(eng, mask, result_fill=-1, heights_fill=-1))
    for out in runs:
        _assert_model(out, name)
        assert out[1].tobytes() == runs[0][1].tobytes()
        assert out[2].tobytes() == runs[0][2].tobytes()


def test_small_wide_small_on_one_engine(eng):
    for name in ("quirk_col0_short_5x4", "stairs_rising_12x8300", "quirk_col0_short_5x4"):
        _assert_model(_native(eng, cc.CASES[name]), name)
    assert cc.CASES["stairs_rising_12x8300"].shape == (12, 8300)


@pytest.mark.parametrize("name", ["quirk_col0_short_5x4", "tie_upper_lower_8x64",
                                  "stairs_falling_12x8300"])
def test_engine_and_stitcher_wrappers(eng, name):
    import torch
    from pano360_amd import stitcher
    mask = cc.CASES[name]
    rect = _model(name)[0][1:5]
    assert eng.crop_rect(torch.from_numpy(np.array(mask)).to(eng.device)) == rect
    y0, x0, h, w = rect
    mosaic = np.random.default_rng(3).integers(0, 256, mask.shape + (3,), dtype=np.uint8)
    for valid in (mask, mask.astype(bool)):
        view = stitcher.crop_mosaic(mosaic, valid)
        assert np.shares_memory(view, mosaic) and view.shape == (h, w, 3)
        assert np.array_equal(view, mosaic[y0:y0 + h, x0:x0 + w])


def test_refusals_write_nothing(eng):
    """PANO_EINVAL, ``result`` and ``heights`` as they were; every buffer is as large as the
    arguments claim.  A valid call on the same context then gives the right answer."""
    small = cc.CASES["quirk_col0_short_5x4"]
    too_wide = np.ones((1, 65537), np.uint8)
    refused = [(small, dict(null=(key,))) for key in ("valid", "heights", "result")]
    refused += [(small, dict(H=0)), (small, dict(W=0)), (too_wide, dict())]
    for mask, kw in refused:
        status, result, heights, mask_after = _native(eng, mask, **kw)
        assert status == EINVAL, kw
        assert np.all(result == SENTINEL) and np.all(heights == SENTINEL), kw
        assert np.array_equal(mask_after, mask), kw
    _assert_model(_native(eng, small), "quirk_col0_short_5x4")
