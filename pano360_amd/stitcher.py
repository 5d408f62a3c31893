"""Drop-in surface of the reference ``stitcher.py`` for the warp/blend/crop path.

Same names, argument order, defaults, return types and side effects as the
reference: ``stitch``, ``no_blend`` / ``linear_blend`` /
``multiband_blend`` (the ``blender(patches, shape)`` protocol; ``median_blend`` and ``seam_blend``
are this port's ghost-rejecting additions to them), ``SphProj``,
``CylProj``, ``_proj_img_range_border``, ``_proj_img_range_corners``,
``estimate_resolution``, ``_hat``, ``_add_weights``, ``_valid``,
``crop_mosaic``, ``find_gains``, ``equalize_gains``, ``BLENDERS``,
``MAX_RESOLUTION`` and the CLI ``main``.
Per-pixel work goes to hand-written HIP kernels through ``_lib`` (ctypes over
``libpano360_hip.so``); there is no CPU fallback for it.

With ``--register`` and no ``ba_<name>.pkl`` the CLI runs the whole chain as the reference's
does (stitcher.py:423-439): feature matching (``features.matching``, cached in
``matches_<name>.npz``), bundle adjustment (``bundle_adj.traverse`` over ``idx_to_keypoints``,
cached in ``ba_<name>.pkl``), then the stitch.  Without the flag a missing camera cache still
ends the run before any image is read.
"""
import argparse
import logging
import os
import pickle
import time

import numpy as np

from . import _lib
from . import bundle_adj as _ba
from . import engine as _eng
from . import fuse as _fuse
from . import lens as _lens
from . import photo as _photo
from .engine import CylProj, SphProj  # noqa: F401  (re-exported API)

MAX_RESOLUTION = 1400       # read at call time, like the reference (stitcher.py:17,154)
# Multiband accuracy contract of ``stitch`` (read at call time; env PANO_EXACT=1 sets the
# default).  False: the fast path - interior pixels take the owner's colour directly (the
# band-pass stack telescopes to it in real arithmetic) and the Gaussian levels run on the
# matrix cores in split float16 - uint8 mosaic within ONE level of the reference wherever
# 255 v sits on an integer boundary (about 1 value in 1000), float mosaic within 1e-4
# relative L2.  True: every pixel through the full band sum and the float32 vector-ALU blur
# (one FMA per tap): the same bounds, but the only deviations left are float32 roundings
# of the blur (<= 1e-6 per plane).  Integer results (valid mask, crop) are exact either way.
EXACT = os.environ.get("PANO_EXACT", "0") not in ("", "0")
_exact_engine = None
# Inlier tolerance of ``median_blend`` per channel, colours in [0, 1] (read at call time;
# ``--ghost-tol``).  Above the exposure and resampling differences between frames of a static
# scene, below the contrast of something that moved; chosen by that reasoning, not tuned on
# photographs.
GHOST_TOL = 0.1
# Zone of ``seam_blend`` (read at call time; ``--seam-ratio``): the seam may move wherever the
# runner-up's weight is at least this share of the owner's.  0.5 - the two weights within a factor
# of two - keeps the seam in the middle half of an overlap of two hat weights, where both frames
# are sampled away from their borders; chosen by that reasoning, not tuned on photographs
# (DESIGN.md section 5t).
SEAM_RATIO = 0.5


def _engine_for_stitch():
    """The process-wide engine, or its exact-mode sibling (vector-ALU blur)."""
    global _exact_engine
    if not EXACT:
        return _eng.engine()
    if _exact_engine is None:
        _exact_engine = _eng.Engine(blur="valu")
    return _exact_engine


# ------------------------------------------------------------------ exposure
def find_gains(overlaps, sizes, stdn=0.1, stdg=2):
    """Find the gains minimizing discrepancies between mean intensities
    (stitcher.py:24-33)."""
    return _eng.find_gains(overlaps, sizes, stdn, stdg)


def _frames_of(regions):
    """uint8 frames behind ``reg.img``: either still uint8 (before
    ``_add_weights``) or the float32 RGBA image ``_add_weights`` made of one, whose
    colours are float32(u8)/255 and convert back exactly."""
    base = np.arange(256, dtype=np.float32) / np.float32(255)
    frames = []
    for reg in regions:
        img = reg.img
        if img.dtype != np.uint8:
            back = np.clip(np.rint(img[..., :3] * np.float32(255)), 0, 255).astype(np.uint8)
            if not np.array_equal(base[back], img[..., :3]):
                raise ValueError("equalize_gains works on frames that came from uint8 images "
                                 "(reg.img as _add_weights leaves it, stitcher.py:257-263)")
            img = back
        frames.append(np.ascontiguousarray(img[..., :3]))
    return frames


def equalize_gains(regions):
    """Equalize the exposures by minimizing differences on overlaps
    (stitcher.py:36-66).  Like the reference it rescales ``reg.img[..., :3]`` of
    float32 RGBA regions in place; the pair statistics run on the GPU
    (``pano_overlap_stats``).  Returns the gains (the reference returns None)."""
    eng = _eng.engine()
    frames = eng.upload_frames(_frames_of(regions))
    _, _, gains, _ = eng.equalize_gains(frames, [r.rot for r in regions],
                                        [r.intr for r in regions])
    for reg, gain in zip(regions, gains):
        if reg.img.dtype != np.uint8:
            reg.img[..., :3] = np.clip(gain * reg.img[..., :3], 0, 1)      # stitcher.py:66
    return gains


# ------------------------------------------------------------ host geometry
def _proj_img_range_border(shape, hom):
    """Extent of a projected frame from its border (stitcher.py:107-122)."""
    return _eng.range_from_border(shape, hom)


def _proj_img_range_corners(shape, hom):
    """Extent from the corners, with wrap-around check (stitcher.py:125-139)."""
    return _eng.range_from_corners(shape, hom)


def estimate_resolution(regions):
    """Resolution of the final image (stitcher.py:142-157)."""
    mid = regions[len(regions) // 2]
    return _eng.resolution_for([reg.range for reg in regions], mid.img.shape[:2],
                               mid.hom(), MAX_RESOLUTION)


def _hat(size):
    """Triangular function of a given size (stitcher.py:251-254)."""
    return _eng.hat(size)


def _add_weights(img):
    """uint8 RGB -> float32 RGBA/255 with alpha = hat(y)*hat(x)
    (stitcher.py:257-263); computed by ``pano_add_weights`` on the GPU."""
    eng = _eng.engine()
    frame = eng.upload_frames([img])[0]
    return eng.add_weights(frame).cpu().numpy()


# ------------------------------------------------------------ patch plumbing
def _upload_patches(eng, patches, n_blur):
    """Host patches of the blender protocol -> device patches (planar planes)."""
    import torch
    out = []
    for warped, mask, irange in patches:
        ys, xs = irange
        dp = _eng.DevicePatch((ys.start, ys.stop, xs.start, xs.stop), eng.device, n_blur)
        src = torch.from_numpy(np.ascontiguousarray(warped, np.float32)).to(eng.device)
        dp.planes[:, :, :dp.w] = src.permute(2, 0, 1)
        if dp.pitch != dp.w:
            dp.planes[:, :, dp.w:] = 0
        dp.mask.copy_(torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)))
        out.append(dp)
    return out


def no_blend(patches, shape):
    """Paste the patches without blending (stitcher.py:160-168)."""
    eng = _eng.engine()
    dev = _upload_patches(eng, patches, 0)
    return eng.simple_blend(dev, tuple(shape), linear=False).cpu().numpy()


def linear_blend(patches, shape):
    """Linearly blend patches (stitcher.py:171-183)."""
    eng = _eng.engine()
    dev = _upload_patches(eng, patches, 0)
    return eng.simple_blend(dev, tuple(shape), linear=True).cpu().numpy()


def multiband_blend(patches, shape, n_levels=5):
    """Multi-band blending (stitcher.py:186-241).  As in the reference, each
    patch's alpha channel is overwritten in place with its sharp ownership
    mask (stitcher.py:207-208)."""
    eng = _eng.engine()
    dev = _upload_patches(eng, patches, n_levels - 1)
    mosaic, _, owner, _ = eng.multiband(dev, tuple(shape), n_levels)
    owner = owner.cpu().numpy()
    for idx, (warped, _, irange) in enumerate(patches):
        warped[..., 3] = owner[irange] == idx
    return mosaic.cpu().numpy()


def median_blend(patches, shape, tol=None):
    """Blend linearly over the samples that agree with the pixel's weighted median sample:
    what moved through the scene in a minority of the frames is voted out, and where nothing
    moved the result is ``linear_blend``'s (no reference counterpart).
    ``tol``: largest difference to the median sample per channel, None = ``GHOST_TOL``."""
    eng = _eng.engine()
    dev = _upload_patches(eng, patches, 0)
    return eng.median_blend(dev, tuple(shape), _ghost_tol(tol)).cpu().numpy()


def seam_blend(patches, shape, n_levels=5, ratio=None):
    """``multiband_blend`` behind a seam finder: inside the zones two frames contest (the
    runner-up's weight at least ``ratio`` of the owner's) the ownership map is rewritten by a
    priority flood over the frames' colour difference, so that the seam runs where the two agree
    and something that only one of them shows is taken from one frame whole (no reference
    counterpart).  ``ratio``: None = ``SEAM_RATIO``.  Like
    ``multiband_blend`` it overwrites each patch's alpha with its sharp ownership mask."""
    eng = _eng.engine()
    dev = _upload_patches(eng, patches, n_levels - 1)
    mosaic, _, owner, _ = eng.seam_multiband(dev, tuple(shape), n_levels, _seam_ratio(ratio))
    owner = owner.cpu().numpy()
    for idx, (warped, _, irange) in enumerate(patches):
        warped[..., 3] = owner[irange] == idx
    return mosaic.cpu().numpy()


def _seam_ratio(ratio=None):
    ratio = SEAM_RATIO if ratio is None else ratio
    if not 0 < ratio <= 1:
        raise ValueError(f"seam_blend: ratio {ratio!r} (0 < ratio <= 1)")
    return float(ratio)


def _ghost_tol(tol=None):
    tol = GHOST_TOL if tol is None else tol
    if not tol >= 0:
        raise ValueError(f"median_blend: tol {tol!r} (>= 0)")
    return float(tol)


BLENDERS = {
    "none": no_blend,
    "linear": linear_blend,
    "multiband": multiband_blend,
    "median": median_blend,
    "seam": seam_blend,
}
_FUSED = {no_blend: "none", linear_blend: "linear", multiband_blend: "multiband",
          median_blend: "median"}


def _valid(patches, shape):
    """Area of validity, OR of ~mask (stitcher.py:266-271)."""
    eng = _eng.engine()
    dev = _upload_patches(eng, patches, 0)
    table = _eng.patch_table(dev, eng)
    _, valid = eng.ownership(table, tuple(shape))
    return valid.cpu().numpy().astype(bool)


def _crop_rect(valid):
    import torch
    eng = _eng.engine()
    dev = torch.from_numpy(np.ascontiguousarray(valid).astype(np.uint8)).to(eng.device)
    rect = eng.crop_rect(dev)
    if rect is None:
        # the reference falls off the end of its scan with `last` unbound
        raise UnboundLocalError("local variable 'last' referenced before assignment")
    return rect


def crop_mosaic(mosaic, valid):
    """Remove the black borders: largest all-valid rectangle with the
    reference's scan-order tie-break; returns a view (stitcher.py:340-369)."""
    y0, x0, h, w = _crop_rect(valid)
    return mosaic[y0:y0 + h, x0:x0 + w, :]


# ------------------------------------------------------------------- stitch
def _download_patches(dev_patches):
    out = []
    for dp in dev_patches:
        y0, y1, x0, x1 = dp.rect
        warped = dp.planes[:, :, :dp.w].permute(1, 2, 0).contiguous().cpu().numpy()
        out.append((warped, dp.mask.cpu().numpy().astype(bool), np.s_[y0:y1, x0:x1]))
    return out


def stitch(regions, blender=no_blend, equalize=False, crop=False, local_align=None):
    """Stitch the images together (stitcher.py:274-327).

    ``regions``: list of ``bundle_adj.Image``.  Side effects kept from the
    reference: ``reg.range`` is filled in and ``reg.img`` is replaced by the
    float32 RGBA weighted image (stitcher.py:277-278).  A blender that is not
    one of this module's three is called with host patches, exactly as the
    reference would call it.

    Accuracy: none / linear and every integer result (valid mask, crop rectangle) equal
    the reference's bit for bit; multiband is within one uint8 level and 1e-4 relative L2
    (see ``EXACT`` above for the two modes).

    ``local_align`` (a ``flow.FlowParams``): the warped patches are aligned locally before the
    blend (``flow.align_device``), and every blender takes the stage path:
    warp, align, blend.  The valid mask and the crop rectangle are those without it.
    """
    if local_align is None:
        return _download_cropped(*_stitch_device(regions, blender, equalize, crop))
    return _download_cropped(*_stitch_device_valid(regions, blender, equalize, crop, False,
                                                   local_align=local_align)[:2])


def _stitch_device(regions, blender, equalize, crop):
    """``stitch`` up to the download: (mosaic, crop rectangle).  The mosaic is the uint8 BGR
    device tensor of the fused blenders (a host array for any other blender); the rectangle is
    (y0, x0, h, w) with ``crop``, else None."""
    return _stitch_device_geometry(regions, blender, equalize, crop)[:2]


def _stitch_device_geometry(regions, blender, equalize, crop, tol=None, ratio=None,
                            local_align=None):
    """``_stitch_device`` and, third, the ``view.MosaicGeometry`` of the whole mosaic (where its
    pixels lie on the sphere: the plan's ``low``, ``resolution`` and ``shape``); the cropped
    mosaic's is ``geometry.cropped(rect)``."""
    return _stitch_device_valid(regions, blender, equalize, crop, False, tol, ratio,
                                local_align)[:3]


def _stitch_device_valid(regions, blender, equalize, crop, want_valid=True, tol=None, ratio=None,
                         local_align=None):
    """``_stitch_device_geometry`` and, fourth, the valid mask the stitch computes (uint8 [H][W] on
    the device, 1 = some frame covers the pixel): ``eng.stitch``'s third result, or
    ``eng.ownership`` of the warped patches for a custom blender, as under ``crop``.  Without
    ``want_valid`` a custom blender's mask is only computed for the crop (else None).  ``tol``:
    ``median_blend``'s tolerance for this stitch (None = ``GHOST_TOL``), ``ratio``: ``seam_blend``'s
    zone (None = ``SEAM_RATIO``); no other blender reads them.  ``seam_blend`` stays on the device
    too, on the stage path: the warped patches go to ``eng.seam_multiband`` as they are.
    ``local_align`` (a ``flow.FlowParams``): every blender takes the stage path, with
    ``eng.flow_align`` between the warp and the blend."""
    from . import view as _view
    eng = _engine_for_stitch()
    frames_host = [reg.img for reg in regions]
    padded = blender == multiband_blend                     # stitcher.py:295
    padded = padded or blender == seam_blend
    plan = _eng.Plan([im.shape[:2] for im in frames_host], [r.rot for r in regions],
                     [r.intr for r in regions], padded, MAX_RESOLUTION)
    frames = eng.upload_frames(frames_host)
    luts = None
    if equalize:                                            # stitcher.py:280-281
        logging.debug("Equalizing gain...")
        luts = eng.equalize_gains(frames, [r.rot for r in regions],
                                  [r.intr for r in regions])[3]
    for i, (reg, rng, frame) in enumerate(zip(regions, plan.ranges, frames)):
        reg.range = rng
        # stitcher.py:277-278 leaves _add_weights' float32 RGBA image in reg.img; our record
        # type fetches it from the device when it is first read (32 x 133 MB for config 3)
        rgba = (lambda f=frame, l=None if luts is None else luts[i]:
                eng.add_weights(f, l).cpu().numpy())
        reg.img = _ba.Deferred(rgba) if isinstance(reg, _ba.Image) else rgba()
    eng.upload_plan(plan)

    kind = _FUSED.get(blender)
    if local_align is not None:
        mosaic, valid, patches = _blend_aligned(eng, frames, plan, luts, blender, kind, local_align,
                                                tol, ratio)
    elif kind is not None:
        n_levels = multiband_blend.__defaults__[0]
        extra = {"tol": _ghost_tol(tol)} if kind == "median" else {}
        mosaic, _, valid, patches = eng.stitch(frames, plan, kind, n_levels, luts=luts,
                                               shortcut=not EXACT, **extra)
    elif blender == seam_blend:
        n_levels = seam_blend.__defaults__[0]
        patches, _ = eng.warp_all(frames, plan, n_blur=n_levels - 1, luts=luts)
        mosaic, _, _, valid = eng.seam_multiband(patches, plan.shape, n_levels, _seam_ratio(ratio))
        moved, n_open, n_groups = (int(v) for v in eng.last_seam_stats[3:6].tolist())
        logging.info(f"Seam routing: {n_groups} groups, {n_open} contested pixels, owner changed "
                     f"on {moved / max(int(valid.sum()), 1):.4f} of the valid pixels")
    else:
        patches, _ = eng.warp_all(frames, plan, luts=luts)
        valid = None
        mosaic = blender(_download_patches(patches), plan.shape)
    rect = None
    if valid is None and (crop or want_valid):
        table = _eng.patch_table(patches, eng)
        _, valid = eng.ownership(table, plan.shape)
    if crop:
        logging.debug("Cropping...")
        rect = eng.crop_rect(valid)
        if rect is None:
            raise UnboundLocalError("local variable 'last' referenced before assignment")
    return mosaic, rect, _view.MosaicGeometry.of_plan(plan), valid


def _blend_aligned(eng, frames, plan, luts, blender, kind, params, tol, ratio):
    """The stage path behind ``local_align``: ``warp_all`` (with the blur planes for multiband and
    seam), ``flow_align``, then the blender's stage call on the aligned patches.  Returns (mosaic,
    valid or None, patches); a custom blender gets the aligned patches downloaded."""
    from . import flow as _flow
    banded = blender in (multiband_blend, seam_blend)
    n_levels = multiband_blend.__defaults__[0]
    patches, _ = eng.warp_all(frames, plan, n_blur=n_levels - 1 if banded else 0, luts=luts)
    patches, stats = eng.flow_align(patches, plan.shape, params)
    _flow.log_statistics(stats)
    valid = None
    if blender == seam_blend:
        mosaic, _, _, valid = eng.seam_multiband(patches, plan.shape, n_levels, _seam_ratio(ratio))
    elif kind == "multiband":
        mosaic, _, _, valid = eng.multiband(patches, plan.shape, n_levels)
    elif kind == "median":
        mosaic = eng.median_blend(patches, plan.shape, _ghost_tol(tol))
    elif kind is not None:
        mosaic = eng.simple_blend(patches, plan.shape, linear=kind == "linear")
    else:
        mosaic = blender(_download_patches(patches), plan.shape)
    return mosaic, valid, patches


def _download_cropped(mosaic, rect):
    """``stitch``'s result: the host mosaic, a view of its crop rectangle when there is one."""
    if hasattr(mosaic, "cpu"):
        mosaic = mosaic.cpu().numpy()
    if rect is not None:
        y0, x0, h, w = rect
        mosaic = mosaic[y0:y0 + h, x0:x0 + w, :]
    return mosaic


# ---------------------------------------------------------------------- CLI
IMAGE_EXTENSIONS = (".jpg", ".png", ".bmp", ".JPG", ".PNG", ".BMP")     # stitcher.py:411-412


def ingest(path, shrink, decode="device", lens=None, bracket=None):
    """The head of the reference's ``main`` (stitcher.py:415-421): every image of the
    directory, in ``os.listdir`` order, as ``cv2.imread`` would return it (uint8 BGR), shrunk by
    ``cv2.resize(im, None, fx=1/shrink, fy=1/shrink)`` when shrink > 1 - on the device.
    decode="device": baseline JPEGs are decoded on the device in one batch
    (``jpeg.read_images``), everything else by Pillow; "host": every file by Pillow.  The frames
    are the same either way.  ``lens`` (a ``lens.Calibration``): every decoded frame's lens
    distortion is corrected on the device, at the file's own resolution, before the shrink.
    ``bracket`` (a ``fuse.Bracket``, or the number of exposures per position): the images are
    taken in sorted file-name order instead, K consecutive files are one position's exposures
    (``fuse.group_files``), and after the one decode every group is fused into one frame by one
    ``fuse.fuse_device`` call - after one ``align.align_device`` call when the bracket has an
    ``align`` (hand-held brackets) and one ``deghost.deghost_device`` call when it has a
    ``deghost`` (something moved between the exposures): decode, align, deghost, fuse, lens,
    shrink; the fused frames take the images' place, in group order, the lens
    correction then runs under each group's first file name: decode, fuse, lens, shrink.
    Returns uint8 [h][w][3] device tensors."""
    from . import blend as _blend
    from . import jpeg as _jpeg
    if decode not in ("device", "host"):
        raise ValueError(f"decode={decode!r}: 'device' or 'host'")
    files = [f for f in os.listdir(path) if any(f.endswith(ext) for ext in IMAGE_EXTENSIONS)]
    groups = None
    if bracket is not None:
        if not isinstance(bracket, _fuse.Bracket):
            bracket = _fuse.Bracket(bracket)
        groups = _fuse.group_files(files, bracket.k)
        files = [f for group in groups for f in group]
    paths = [os.path.join(path, f) for f in files]
    if decode == "host":
        # cv2.imread's defaults: the EXIF orientation applied (a phone's rotated JPEG arrives
        # upright, with its shape swapped), 8 bits, three channels: 16-bit images are scaled
        # down to 8 bits and an alpha channel is dropped, as IMREAD_COLOR does
        images = [_jpeg._pillow_read(p) for p in paths]
        if lens is None and groups is None:
            return _blend.shrink_images(images, shrink)
        frames = _blend.shrink_images(images, 1)            # (the upload alone)
    else:
        frames, _ = _jpeg.read_images(paths)
    if groups is not None:
        frames = bracket.fuse_groups(frames, groups)
        files = [group[0] for group in groups]
    if lens is not None:
        frames = lens.correct_device(frames, files)
    if shrink > 1:
        eng = _eng.engine()
        frames = [_blend.shrink_device(f, shrink, eng) for f in frames]
    return frames


def idx_to_keypoints(matches, kpts):
    """The match file's keypoint indices replaced by homogeneous coordinates
    (stitcher.py:372-386): ``matches`` the 0-d object array of ``matches_<name>.npz`` ([i][j] =
    (int [M][2] (index in i, index in j), homography i -> j)), ``kpts`` the keypoint arrays.
    Returns {i: {j: (float64 [M][6] (x_i, y_i, 1, x_j, y_j, 1), homography, M)}}, what
    ``bundle_adj.traverse`` takes."""
    hom_kpts = [np.concatenate([kp, np.ones((kp.shape[0], 1))], axis=1) for kp in kpts]
    table = matches.item() if isinstance(matches, np.ndarray) else matches
    return {i: {j: (np.concatenate([hom_kpts[i][m[:, 0]], hom_kpts[j][m[:, 1]]], axis=1), h,
                    len(m))
                for j, (m, h) in row.items()}
            for i, row in table.items()}


def _register(path, name, frames, badjust, detector="sift"):
    """Cameras for the frames of ``path`` (stitcher.py:423-439): the match file is read if
    present, else ``features.matching`` runs on the device frames and writes it; then
    ``traverse``, whose cameras are pickled with host uint8 BGR images so that the reference
    CLI reads the cache too.  Returns the cameras with the device frames attached.
    ``detector`` "msop" matches with ``features.msop_detector()``; ``name`` then carries the
    ``_msop`` suffix that keeps its caches apart from SIFT's."""
    from . import features
    try:
        arr = np.load(f"matches_{name}.npz", allow_pickle=True)
        kpts, matches = arr["kpts"], arr["matches"]
    except IOError:
        kpts, matches = features.matching(frames, **features.detector_kwargs(detector))
        np.savez(f"matches_{name}.npz", kpts=kpts, matches=matches)
    start = time.time()
    regions = _ba.traverse(list(frames), idx_to_keypoints(matches, kpts), badjust=badjust)
    logging.info(f"Image registration, time: {time.time() - start}")
    device = [reg.img for reg in regions]
    for reg, frame in zip(regions, device):
        reg.img = frame.cpu().numpy() if hasattr(frame, "cpu") else np.asarray(frame)
    with open(f"ba_{name}.pkl", "wb") as fid:
        pickle.dump(regions, fid, protocol=pickle.HIGHEST_PROTOCOL)
    for reg, frame in zip(regions, device):
        reg.img = frame
    return regions


def _image_index(regions, frames):
    """The image number of every camera ``traverse`` returned: it attaches ``frames[i]`` itself
    to camera i and leaves out the images it did not reach."""
    return [next(i for i, frame in enumerate(frames) if frame is reg.img) for reg in regions]


REFINE_MIN_SHARE = 0.5      # of the matches within the threshold, for a refinement to be used


def _refine(regions, name, index, lens_terms):
    """``--refine`` / ``--refine-lens``: ``bundle_adj.refine`` of the cameras in hand over the
    matches of ``matches_<name>.npz`` and, with ``lens_terms``, the correction of their frames by
    the fitted distortion (``lens.undistort_device``: cubic, the fitted focal length, which
    becomes the camera's).  Returns the new regions - or, when fewer than REFINE_MIN_SHARE of the
    matches end within the threshold, the regions given, with a warning."""
    try:
        arr = np.load(f"matches_{name}.npz", allow_pickle=True)
    except IOError:
        raise SystemExit(f"--refine needs the matches of matches_{name}.npz, which is missing: "
                         "run with --register (and without a camera cache) to write it") from None
    kpts, matches = arr["kpts"], arr["matches"]
    if index is None:
        if len(regions) != len(kpts):
            raise SystemExit(f"ba_{name}.pkl holds {len(regions)} cameras for the {len(kpts)} "
                             f"images of matches_{name}.npz and does not say which: remove it "
                             "and run --register and --refine in one call")
        index = range(len(regions))
    start = time.time()
    res = _ba.refine(regions, idx_to_keypoints(matches, kpts), list(index),
                     lens_terms=lens_terms or 0)
    focals = ", ".join(f"{reg.intr[0, 0]:.3f}" for reg in res.cameras)
    logging.info(f"Refinement, time: {time.time() - start}: rms {res.rms_before:.4f} -> "
                 f"{res.rms_after:.4f} px over the matches within the threshold, inlier share "
                 f"{res.inlier_share:.4f}, k = ({res.k[0]:.6g}, {res.k[1]:.6g}), focal lengths "
                 f"{focals}")
    if res.inlier_share < REFINE_MIN_SHARE:
        # the loop is local: from cameras too far off it can end anywhere, and a distortion
        # fitted there would bend every frame
        logging.warning(f"Refinement discarded: only {res.inlier_share:.2f} of the matches end "
                        "within the threshold, so the cameras it started from were too far off; "
                        "the cameras and the frames stay as they were")
        return regions
    regions = res.cameras
    if lens_terms:
        frames = [reg.img for reg in regions]
        models = res.lens_models([(f.shape[1], f.shape[0]) for f in frames])
        frames, focals = _lens.undistort_device(frames, models, "cubic")
        for reg, frame, focal in zip(regions, frames, focals):
            reg.img, reg.intr = frame, _ba.intrinsics(focal)
    return regions


def _view_spec(text):
    """``YAW,PITCH,FOV[,WxH]`` of --view, degrees: (yaw, pitch, fov, (w, h))."""
    parts = text.split(",")
    try:
        if len(parts) not in (3, 4):
            raise ValueError(text)
        yaw, pitch, fov = (float(v) for v in parts[:3])
        w, h = (int(v) for v in parts[3].lower().split("x")) if len(parts) == 4 else (1920, 1080)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: YAW,PITCH,FOV[,WxH]") from None
    if not 0 < fov < 180 or w < 1 or h < 1:
        raise argparse.ArgumentTypeError(f"{text!r}: 0 < FOV < 180 degrees, sides >= 1")
    return yaw, pitch, fov, (w, h)


def _positive(text):
    value = int(text)
    if value < 1:
        raise argparse.ArgumentTypeError(f"{text}: >= 1")
    return value


def _tolerance(text):
    value = float(text)
    if not value >= 0:
        raise argparse.ArgumentTypeError(f"{text}: >= 0")
    return value


def _zone_ratio(text):
    value = float(text)
    if not 0 < value <= 1:
        raise argparse.ArgumentTypeError(f"{text}: in (0, 1]")
    return value


def local_align_of(args):
    """The ``flow.FlowParams`` that ``--local-align`` and ``--local-align-levels`` ask for, or
    None."""
    if not getattr(args, "local_align", False):
        return None
    from . import flow as _flow
    return _flow.FlowParams(levels=getattr(args, "local_align_levels", 3))


def refine_of(args):
    """(whether to refine, the radial terms to fit or None): what ``--refine`` and
    ``--refine-lens`` asked for."""
    terms = getattr(args, "refine_lens", None)
    return bool(getattr(args, "refine", False)) or terms is not None, terms


def parse_args(argv=None):
    """The reference's command line (stitcher.py:390-409) and this port's additions."""
    parser = argparse.ArgumentParser(description="Stitch images.")
    parser.add_argument("path", type=str, help="directory with the images to process.")
    parser.add_argument("-s", "--shrink", type=float, default=2,
                        help="downsample the images by this amount.")
    parser.add_argument("--ba", default="incr", choices=["none", "incr", "last"],
                        help="bundle adjustment type.")
    parser.add_argument("--equalize", "-e", action="store_true",
                        help="equalize image gain before stitching.")
    parser.add_argument("--crop", "-c", action="store_true", help="remove the black borders.")
    parser.add_argument("--blend", "-b", default="multiband", choices=list(BLENDERS.keys()),
                        help="blending algorithm.")
    parser.add_argument("--ghost-tol", type=_tolerance, metavar="FLOAT",
                        help="-b median: a frame's sample counts where every channel is within "
                             f"this of the pixel's median sample (colours in [0, 1]; default "
                             f"{GHOST_TOL}).")
    # (an absent flag leaves no attribute: the parsed namespace without it is what it was)
    parser.add_argument("--seam-ratio", type=_zone_ratio, metavar="FLOAT", default=argparse.SUPPRESS,
                        help="-b seam: the seam may move wherever the runner-up frame's weight is "
                             f"at least this share of the owner's (in (0, 1]; default {SEAM_RATIO}).")
    parser.add_argument("--local-align", action="store_true", default=argparse.SUPPRESS,
                        help="align overlapping frames locally before the blend: what a hand-held "
                             "sweep's parallax doubles is moved to where the frames meet (every "
                             "blender; DESIGN.md section 5u).")
    parser.add_argument("--local-align-levels", type=int, choices=range(_lib.FLOW_MAX_LEVELS + 1),
                        default=argparse.SUPPRESS, metavar="N",
                        help="--local-align: pyramid levels of the search, a reach of "
                             "2^(N+1) - 1 pixels (0 .. 4; default 3).")
    parser.add_argument("-o", "--out", type=str, help="save result to this file")
    parser.add_argument("--register", action="store_true",
                        help="without a camera cache, match the images and run bundle "
                             "adjustment (writes matches_<name>.npz and ba_<name>.pkl)")
    parser.add_argument("--detector", default="sift", choices=["sift", "msop"],
                        help="feature detector of --register (msop: the caches are named "
                             "matches_<name>_msop.npz and ba_<name>_msop.pkl).")
    parser.add_argument("--view", action="append", type=_view_spec, default=[],
                        metavar="YAW,PITCH,FOV[,WxH]",
                        help="also save a pinhole look at the mosaic (degrees; default 1920x1080) "
                             "as <out>_view<k>; repeatable; a negative yaw is written --view=-30,0,90.")
    parser.add_argument("--equirect", type=_positive, metavar="WIDTH",
                        help="also save the full-sphere 2:1 equirectangular image as "
                             "<out>_equirect.")
    parser.add_argument("--cube", type=_positive, metavar="SIDE",
                        help="also save the six cube faces as <out>_cube_<face>.")
    parser.add_argument("--deepzoom", action="store_true",
                        help="also save the mosaic as a Deep Zoom tile pyramid: <out>.dzi and "
                             "<out>_files/.")
    parser.add_argument("--multires", type=_positive, metavar="SIDE",
                        help="also save the sphere as a multiresolution cube of at most this "
                             "side, with its config.json, in <out>_multires/.")
    parser.add_argument("--tile", type=_positive, default=512, metavar="N",
                        help="tile side of --deepzoom and --multires (default 512).")
    parser.add_argument("--fill", action="store_true",
                        help="fill what no frame covers from the pixels around it: the saved "
                             "mosaic and --deepzoom show no ragged border, and --view, --equirect, "
                             "--cube and --multires no black outside the mosaic (not with --crop).")
    # (absent flags leave no attribute: the parsed namespace without them is what it was)
    parser.add_argument("--refine", action="store_true", default=argparse.SUPPRESS,
                        help="refine the cameras robustly after the registration or the camera "
                             "cache (bundle_adj.refine over matches_<name>.npz); recomputed on "
                             "every run, no cache changes.")
    parser.add_argument("--refine-lens", type=int, choices=[1, 2], default=argparse.SUPPRESS,
                        metavar="{1,2}",
                        help="--refine that also fits 1 (k1) or 2 (k1, k2) radial distortion "
                             "terms shared by all images, and corrects the images by them before "
                             "the stitch (not with --lens).")
    _lens.add_arguments(parser)
    _photo.add_arguments(parser)
    _fuse.add_arguments(parser)
    args = parser.parse_args(argv)
    if refine_of(args)[1] is not None:
        if args.lens is not None:
            parser.error("--refine-lens and --lens both set the lens: give one of them")
        args.refine = True
    _lens.check_arguments(parser, args)
    _photo.check_arguments(parser, args)
    _fuse.check_arguments(parser, args)
    if args.ghost_tol is not None and args.blend != "median":
        parser.error("--ghost-tol needs -b median")
    if hasattr(args, "seam_ratio") and args.blend != "seam":
        parser.error("--seam-ratio needs -b seam")
    if hasattr(args, "local_align_levels") and not hasattr(args, "local_align"):
        parser.error("--local-align-levels needs --local-align")
    if args.fill and args.crop:
        parser.error("--fill and --crop exclude each other: a cropped mosaic has nothing to fill")
    if (args.view or args.equirect or args.cube) and not args.out:
        parser.error("--view, --equirect and --cube need -o")
    if (args.deepzoom or args.multires) and not args.out:
        parser.error("--deepzoom and --multires need -o")
    if args.multires and args.multires < args.tile:
        parser.error("--multires: a side of at least --tile")
    if args.equirect and args.equirect % 2:
        parser.error("--equirect: an even width")
    return args


def cache_name(args):
    """``<name>`` of ``matches_<name>.npz`` and ``ba_<name>.pkl``: the directory and the shrink
    as in the reference, ``_msop`` for that detector, ``_b<K>`` with ``--bracket K`` (``_b<K>a``
    with ``--bracket-align``, ``_b<K>g`` with ``--bracket-deghost``, ``_b<K>ag`` with both),
    ``_lens`` with ``--lens``: matches and cameras of corrected and uncorrected, fused and plain,
    aligned and unaligned, deghosted and ghosted frames never mix."""
    name = f"{os.path.basename(os.path.normpath(args.path))}_s{args.shrink}"
    if args.detector == "msop":
        name += "_msop"
    name += _fuse.cache_suffix(args)
    if args.lens is not None:
        name += "_lens"
    return name


def main(argv=None):
    """Same command line as the reference (stitcher.py:390-451)."""
    args = parse_args(argv)

    name = cache_name(args)
    lens = _lens.from_args(args)
    bracket = _fuse.from_args(args)
    cache = f"ba_{name}.pkl"
    try:
        with open(cache, "rb") as fid:
            regions = pickle.load(fid)
    except IOError:
        regions = None
    # stitcher.py:415-421: list the directory (os.listdir order, the reference's extensions),
    # read, shrink.  The reference does this before it looks at its caches and, with a
    # ``ba_*.pkl`` present, never uses the result (the pickle carries the shrunk images); here
    # the images are read only when something consumes them: a cache without pixels
    # (``img=None`` records: cameras only, a few hundred bytes per frame) or, with --register,
    # no cache at all: then the frames are matched and registered and go to the stitch as
    # they are.
    # Baseline JPEGs are decoded on the device (``jpeg.read_images``), other files by Pillow;
    # the resize runs on the device (``pano_resize_u8``) and the frames stay there for ``stitch``.
    if regions is None and not args.register:
        # (before anything is decoded or uploaded)
        raise SystemExit(
            f"{cache} not found: run with --register to match the images and adjust the "
            "cameras here (the reference CLI's registration), or produce the camera cache with "
            "the reference (the pickle written at stitcher.py:438-439) and re-run")
    index = None                    # of a cache: camera k is image k, if their numbers agree
    if regions is None:
        frames = ingest(args.path, args.shrink, lens=lens, bracket=bracket)
        regions = _register(args.path, name, frames, args.ba, args.detector)
        index = _image_index(regions, frames)
    if any(reg.img is None for reg in regions):
        frames = ingest(args.path, args.shrink, lens=lens, bracket=bracket) \
            if os.path.isdir(args.path) else []
        if len(frames) != len(regions):
            raise SystemExit(f"{cache} holds {len(regions)} cameras, {args.path} "
                             f"{len(frames)} images")
        for reg, frame in zip(regions, frames):
            if reg.img is None:
                reg.img = frame
    if refine_of(args)[0]:
        # refine -> undistort -> --photometric -> stitch
        regions = _refine(regions, name, index, refine_of(args)[1])
    if _photo.mode_of(args) is not None:
        # after the registration, which sees the frames as they are (no cache name changes),
        # and before the stitch: every blender, --crop, --fill, the views and the tiles get
        # the corrected frames
        start = time.time()
        _photo.correct_regions(regions, _photo.MODES[_photo.mode_of(args)])
        logging.info(f"Photometric alignment, time: {time.time() - start}")

    start = time.time()
    background = None
    if args.fill:
        dev_mosaic, rect, geom, valid = _stitch_device_valid(regions, BLENDERS[args.blend],
                                                             args.equalize, False,
                                                             tol=args.ghost_tol,
                                                             ratio=getattr(args, "seam_ratio", None),
                                                             local_align=local_align_of(args))
        dev_mosaic, background = _filled(args, dev_mosaic, geom, valid)
    else:
        dev_mosaic, rect, geom = _stitch_device_geometry(regions, BLENDERS[args.blend],
                                                         args.equalize, args.crop,
                                                         tol=args.ghost_tol,
                                                         ratio=getattr(args, "seam_ratio", None),
                                                         local_align=local_align_of(args))
    mosaic = _download_cropped(dev_mosaic, rect)
    logging.info(f"Built mosaic, time: {time.time() - start}")
    if args.out:
        _save(args.out, dev_mosaic, rect, mosaic)
        _save_views(args, dev_mosaic, rect, geom, background)
        _save_tiles(args, dev_mosaic, rect, geom, background)
    return mosaic


def _filled(args, dev_mosaic, geom, valid):
    """--fill: the mosaic with its uncovered pixels filled (``fill.fill_device``; a custom
    blender's host mosaic is uploaded) and, when a view of the sphere is asked for, the background
    those views are composited over: (``view.Mips``, geometry) of ``fill.sphere_device``."""
    from . import fill as _fill
    from . import view as _view
    start = time.time()
    filled = _fill.fill_device(dev_mosaic, valid, geom.closed)
    background = None
    if args.out and (args.view or args.equirect or args.cube or args.multires):
        sphere, sphere_geom = _fill.sphere_device(filled, geom)
        background = (_view.mip_device(sphere), sphere_geom)
    logging.info(f"Filled the mosaic, time: {time.time() - start}")
    return filled, background


def view_outputs(args):
    """[(file name, view)] of --view, --equirect and --cube: ``<stem>_view<k><ext>``,
    ``<stem>_equirect<ext>``, ``<stem>_cube_<face><ext>`` beside ``args.out``."""
    from . import view as _view
    stem, ext = os.path.splitext(args.out)
    rad = np.pi / 180
    out = [(f"{stem}_view{k}{ext}", _view.perspective(yaw * rad, pitch * rad, 0.0, fov * rad, size))
           for k, (yaw, pitch, fov, size) in enumerate(args.view)]
    if args.equirect:
        out.append((f"{stem}_equirect{ext}", _view.equirect(args.equirect)))
    if args.cube:
        out += [(f"{stem}_cube_{face}{ext}", v)
                for face, v in zip(_view.CUBE_FACES, _view.cube_faces(args.cube))]
    return out


def _save_views(args, dev_mosaic, rect, geom, background=None):
    """Renders the views the command line asks for from the mosaic (the cropped one with --crop;
    a custom blender's host mosaic is uploaded) in one launch, and writes them like the mosaic.
    ``background`` (--fill): what the mosaic does not cover comes from that sphere."""
    from . import view as _view
    outputs = view_outputs(args)
    if not outputs:
        return
    start = time.time()
    if rect is not None:
        y0, x0, h, w = rect
        dev_mosaic, geom = dev_mosaic[y0:y0 + h, x0:x0 + w, :], geom.cropped(rect)
    if background is None:
        images, _ = _view.render_device(dev_mosaic, geom, [v for _, v in outputs])
    else:
        from . import fill as _fill
        images, _ = _fill.render_filled_device(dev_mosaic, geom, [v for _, v in outputs], background)
    for (path, _), image in zip(outputs, images):
        _save(path, image, None, None)
    logging.info(f"Rendered {len(outputs)} views, time: {time.time() - start}")


def _save_tiles(args, dev_mosaic, rect, geom, background=None):
    """The tile pyramids the command line asks for (``tiles.write_deepzoom``: ``<stem>.dzi`` and
    ``<stem>_files/``; ``tiles.write_multires``: ``<stem>_multires/``), from the mosaic
    ``_save_views`` uses, through one mip chain."""
    if not (args.deepzoom or args.multires):
        return
    from . import tiles as _tiles
    from . import view as _view
    start = time.time()
    if rect is not None:
        y0, x0, h, w = rect
        dev_mosaic, geom = dev_mosaic[y0:y0 + h, x0:x0 + w, :], geom.cropped(rect)
    stem = os.path.splitext(args.out)[0]
    mips = _view.mip_device(dev_mosaic)
    written = []
    if args.deepzoom:
        written += _tiles.write_deepzoom(stem, mips, args.tile)
    if args.multires:
        written += _tiles.write_multires(f"{stem}_multires", mips, geom, args.multires, args.tile,
                                         background=background)
    logging.info(f"Wrote {len(written)} tile files, time: {time.time() - start}")


def _save(path, dev_mosaic, rect, mosaic):
    """Write the mosaic as Pillow's ``save(path)`` would.  A JPEG of a device mosaic is
    encoded on the device at Pillow's defaults (``jpeg.encode_device``: the same bytes), a PNG
    of one by ``png.encode_device`` (the same pixels, not zlib's bytes); every other format,
    and the host mosaic of a custom blender, goes through Pillow (``mosaic`` None: the device
    image is downloaded for it)."""
    from . import jpeg as _jpeg
    from . import png as _png
    lower = path.lower()
    codec = _jpeg if lower.endswith(_jpeg.JPEG_EXTENSIONS) else \
        _png if lower.endswith(_png.PNG_EXTENSIONS) else None
    if codec is not None and hasattr(dev_mosaic, "cpu"):
        view = dev_mosaic
        if rect is not None:
            y0, x0, h, w = rect
            view = dev_mosaic[y0:y0 + h, x0:x0 + w, :]
        if codec.encodable(view):
            data = codec.encode_device(view, order="bgr")
            with open(path, "wb") as fid:
                fid.write(data)
            return
    from PIL import Image as PilImage
    if mosaic is None:
        mosaic = dev_mosaic.cpu().numpy()
    PilImage.fromarray(np.ascontiguousarray(mosaic[..., ::-1])).save(path)


if __name__ == "__main__":
    logging.basicConfig(level=logging.DEBUG)
    main()
