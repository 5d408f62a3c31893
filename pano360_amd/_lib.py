"""ctypes binding of ``libpano360_hip.so`` (declared in ``include/pano360.h``).

There is no CPU fallback: if the library is missing or a call fails the caller
gets an exception.  ``torch`` is imported first so that the HIP runtime torch
ships is the one both sides use (the library is linked against the SONAME
``libamdhip64.so.7``, which the loader then resolves to the already loaded
copy); torch itself is only used for device memory, streams and
``torch.distributed``.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PANO_LIB: another build of the same library (A/B timing of kernel variants)
LIB_PATH = os.environ.get("PANO_LIB") or os.path.join(_HERE, "libpano360_hip.so")

# The PANO_X macros of include/pano360.h that the package uses, each as X; the package states them
# nowhere else (tests/test_host_abi.py compares every one with the C compiler's value)
MAX_TAPS = 129
MAX_LEVELS = 8
TAP_LEAD = 7
TAP_PAD = 40
# pano_ctx options
OPT_BLUR_KERNEL, OPT_OWN_PRUNE, OPT_BLUR_SEGMENTS, OPT_BLUR_LEAN, OPT_STITCH_STREAMS = 0, 1, 2, 3, 4
OPT_STITCH_ASYNC = 5
OPT_BLUR_SEG_LEN = 6
OPT_SIFT_GRAPH = 7
OPT_LEVEL_CLASSES = 8
BLUR_MFMA, BLUR_VALU = 0, 1


class PanoError(RuntimeError):
    """A C-ABI call returned a negative status."""


class Patch(C.Structure):
    """``pano_patch`` of include/pano360.h (96 bytes)."""
    _fields_ = [("planes", C.c_void_p), ("mask", C.c_void_p),
                ("blurred", C.c_void_p), ("scratch", C.c_void_p),
                ("y0", C.c_int32), ("x0", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("vy0", C.c_int32), ("vx0", C.c_int32), ("vh", C.c_int32), ("vw", C.c_int32),
                ("ay0", C.c_int32), ("ax0", C.c_int32), ("ah", C.c_int32), ("aw", C.c_int32),
                ("vpitch", C.c_int32), ("apitch", C.c_int32),
                ("index", C.c_int32), ("tiles_off", C.c_int32)]


class Layout(C.Structure):
    """``pano_layout`` of include/pano360.h."""
    _fields_ = [("planes_floats", C.c_int64), ("blurred_floats", C.c_int64),
                ("scratch_floats", C.c_int64), ("n_records", C.c_int32), ("n_tiles", C.c_int32),
                ("max_vw", C.c_int32), ("max_vh", C.c_int32), ("max_aw", C.c_int32),
                ("max_ah", C.c_int32), ("missing", C.c_int32)]


class SiftArgs(C.Structure):
    """``pano_sift_args`` of include/pano360.h."""
    _fields_ = [("frame", C.c_void_p), ("frame_copy", C.c_void_p),
                ("h", C.c_int32), ("w", C.c_int32), ("n_octaves", C.c_int32), ("n_layers", C.c_int32),
                ("taps", C.c_void_p), ("ntaps", C.c_void_p), ("gauss", C.c_void_p),
                ("dog", C.c_void_p), ("work", C.c_void_p), ("detect", C.c_int32),
                ("contrast_thr", C.c_float), ("edge_thr", C.c_float), ("sigma", C.c_float),
                ("first_octave", C.c_int32), ("max_keypoints", C.c_int32),
                ("gauss_dev", C.c_void_p), ("dims_dev", C.c_void_p), ("cands", C.c_void_p),
                ("kpts", C.c_void_p), ("counts", C.c_void_p), ("sort_work", C.c_void_p),
                ("desc", C.c_void_p)]


class StitchArgs(C.Structure):
    """``pano_stitch_args`` of include/pano360.h."""
    _fields_ = ([(k, C.c_void_p) for k in (
        "cams", "rects", "have", "sin_t", "cos_t", "tan_p", "lut", "taps", "ntaps", "owner",
        "valid", "marks", "regions", "regions_host", "block_owner", "interior", "records_host",
        "table", "planes", "blurred", "scratch", "tile_flags", "need", "mosaic", "mosaic_f32")]
        + [(k, C.c_int64) for k in ("planes_floats", "blurred_floats", "scratch_floats")]
        + [(k, C.c_int32) for k in (
            "n", "H", "W", "xs0", "xs1", "own0", "own1", "lut_stride", "n_levels", "radius",
            "shortcut", "warp_need", "max_spans", "min_gap", "cap_records", "cap_tiles",
            "used_need", "trust_layout")]
        + [("classes", C.c_void_p), ("layout", Layout)])


EINVAL = -1     # PANO_EINVAL
ESOLVE = -4     # PANO_ESOLVE: pano_poisson_blend did not converge (cap or breakdown)
EGROW = 1       # pano_stitch_multiband: an arena is too small, args.layout says what is needed
# pano_stitch_args.trust_layout: what the caller asks for, and what the stitch did
TRUST_NONE, TRUST_LAYOUT, TRUST_GEOMETRY = 0, 1, 3
TRUST_TRUSTED, TRUST_KEPT = 2, 4
# pano_seam_levels' dtype codes, the resident flood's capacity in cells (wall included)
SEAM_U8, SEAM_I16, SEAM_I32, SEAM_F32, SEAM_F64 = 0, 1, 2, 3, 4
SEAM_DTYPES = {"uint8": SEAM_U8, "int16": SEAM_I16, "int32": SEAM_I32, "float32": SEAM_F32,
               "float64": SEAM_F64}
SEAM_RESIDENT_CELLS = 81408
# pano_seam_route_prepare / pano_seam_route: the cameras the pair matrix holds
SEAM_ROUTE_MAX_CAMERAS = 4096
# pano_flow_*: levels, the pairs a candidate needs, gain
FLOW_MAX_LEVELS, FLOW_MIN_COUNT, FLOW_MAX_GAIN = 4, 128, 4080
# pano_ssc_probe's paths, the on-chip bitmap's capacity in cells
SSC_AUTO, SSC_ONCHIP, SSC_GLOBAL = 0, 1, 2
SSC_ONCHIP_CELLS = 524288
# pano_ba_refine: the sums per pair (the header states the figure in prose only)
BA_REFINE_TERMS = 70
# pano_jpeg_decode: int64 fields of a descriptor row, entropy bytes per destuffing thread, bits
# per Huffman subsequence, bytes of one lookup table
JPEG_FIELDS = 32
JPEG_CHUNK = 1024
JPEG_SUBSEQ = 1024
JPEG_HUFF_BYTES = 1424
# pano_jpeg_encode / pano_jpeg_encode_batch: the largest side, the flag "pixels are B, G, R"
JPEG_MAX_SIDE = 65500
JPEG_BGR = 1
JPEG_BATCH_MAX = 16384
JPEG_BATCH_MAX_BLOCKS = 1 << 28
# pano_png_filter's flag; pano_deflate: input bytes per block, the first length it refuses
PNG_BGR = 1
DEFLATE_CHUNK = 65536
DEFLATE_MAX_BYTES = 1 << 34
# pano_mip_u8 / pano_view_render: the limits, the kinds of a view
VIEW_MAX_LEVELS = 16
VIEW_MAX_VIEWS = 32
VIEW_MAX_SIDE = 32768
VIEW_RECTILINEAR, VIEW_EQUIRECT, VIEW_STEREOGRAPHIC = 0, 1, 2
# pano_median_cameras / pano_median_blend
MEDIAN_KEEP = 32
# pano_fill_u8
FILL_TAIL_PIXELS = 4096
# pano_lens_undistort_u8: the largest side, the models and interpolations
LENS_MAX_SIDE = 32767
LENS_BROWN, LENS_FISHEYE = 0, 1
LENS_CUBIC, LENS_LINEAR = 0, 1
# pano_photo_stats / pano_photo_apply_u8
PHOTO_MAX_SIDE = 32767
PHOTO_SUMS = 25
PHOTO_TABLE = 1026
# pano_fuse_u8 / pano_align_mtb / pano_deghost_u8
FUSE_MAX_EXPOSURES = 8
FUSE_MAX_SIDE = 32767


class JpegImage(C.Structure):
    """``pano_jpeg_image`` of include/pano360.h (24 bytes)."""
    _fields_ = [("img", C.c_void_p), ("pitch", C.c_int64), ("h", C.c_int32), ("w", C.c_int32)]


class View(C.Structure):
    """``pano_view`` of include/pano360.h (136 bytes)."""
    _fields_ = [("m", C.c_double * 9), ("p", C.c_double * 4),
                ("image", C.c_void_p), ("mask", C.c_void_p),
                ("kind", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("reserved", C.c_int32)]


class ViewMosaic(C.Structure):
    """``pano_view_mosaic`` of include/pano360.h (48 bytes)."""
    _fields_ = [("low", C.c_double * 2), ("res", C.c_double * 2),
                ("h", C.c_int32), ("w", C.c_int32), ("closed", C.c_int32),
                ("reserved", C.c_int32)]


class LensFrame(C.Structure):
    """``pano_lens_frame`` of include/pano360.h (128 bytes)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p),
                ("src_pitch", C.c_int64), ("dst_pitch", C.c_int64),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("f_new", C.c_double), ("k", C.c_double * 5),
                ("w", C.c_int32), ("h", C.c_int32), ("model", C.c_int32), ("interp", C.c_int32)]


class PhotoFrame(C.Structure):
    """``pano_photo_frame`` of include/pano360.h (24 bytes)."""
    _fields_ = [("img", C.c_void_p), ("pitch", C.c_int64), ("w", C.c_int32), ("h", C.c_int32)]


class PhotoPair(C.Structure):
    """``pano_photo_pair`` of include/pano360.h (80 bytes)."""
    _fields_ = [("H", C.c_double * 9), ("i", C.c_int32), ("j", C.c_int32)]


class PhotoApply(C.Structure):
    """``pano_photo_apply`` of include/pano360.h (48 bytes)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("table", C.c_void_p),
                ("src_pitch", C.c_int64), ("dst_pitch", C.c_int64),
                ("w", C.c_int32), ("h", C.c_int32)]


class FuseStack(C.Structure):
    """``pano_fuse_stack`` of include/pano360.h (176 bytes)."""
    _fields_ = [("src", C.c_void_p * FUSE_MAX_EXPOSURES), ("src_pitch", C.c_int64 * FUSE_MAX_EXPOSURES),
                ("dst", C.c_void_p), ("dst_pitch", C.c_int64),
                ("raw", C.c_void_p), ("fused", C.c_void_p),
                ("w", C.c_int32), ("h", C.c_int32), ("k", C.c_int32), ("reserved", C.c_int32)]


class FuseParams(C.Structure):
    """``pano_fuse_params`` of include/pano360.h (16 bytes)."""
    _fields_ = [("contrast", C.c_float), ("saturation", C.c_float), ("exposure", C.c_float),
                ("n_levels", C.c_int32)]


class AlignStack(C.Structure):
    """``pano_align_stack`` of include/pano360.h (312 bytes)."""
    _fields_ = [("src", C.c_void_p * FUSE_MAX_EXPOSURES), ("src_pitch", C.c_int64 * FUSE_MAX_EXPOSURES),
                ("dst", C.c_void_p * FUSE_MAX_EXPOSURES), ("dst_pitch", C.c_int64 * FUSE_MAX_EXPOSURES),
                ("shifts", C.c_void_p), ("grey", C.c_void_p), ("medians", C.c_void_p),
                ("bitmaps", C.c_void_p), ("errs", C.c_void_p),
                ("w", C.c_int32), ("h", C.c_int32), ("k", C.c_int32), ("reference", C.c_int32)]


class AlignParams(C.Structure):
    """``pano_align_params`` of include/pano360.h (8 bytes)."""
    _fields_ = [("max_bits", C.c_int32), ("exclude", C.c_int32)]


class FlowParams(C.Structure):
    """``pano_flow_params`` of include/pano360.h (16 bytes)."""
    _fields_ = [("levels", C.c_int32), ("gain", C.c_int32), ("min_overlap", C.c_int32),
                ("reserved", C.c_int32)]


class DeghostStack(C.Structure):
    """``pano_deghost_stack`` of include/pano360.h (320 bytes)."""
    _fields_ = [("src", C.c_void_p * FUSE_MAX_EXPOSURES), ("src_pitch", C.c_int64 * FUSE_MAX_EXPOSURES),
                ("dst", C.c_void_p * FUSE_MAX_EXPOSURES), ("dst_pitch", C.c_int64 * FUSE_MAX_EXPOSURES),
                ("counts", C.c_void_p), ("hists", C.c_void_p), ("ranks", C.c_void_p), ("maps", C.c_void_p),
                ("raw", C.c_void_p), ("mask", C.c_void_p),
                ("w", C.c_int32), ("h", C.c_int32), ("k", C.c_int32), ("reference", C.c_int32)]


class DeghostParams(C.Structure):
    """``pano_deghost_params`` of include/pano360.h (16 bytes)."""
    _fields_ = [("slack", C.c_int32), ("tol", C.c_int32), ("erode", C.c_int32), ("dilate", C.c_int32)]


class Pair(C.Structure):
    """``pano_pair`` of include/pano360.h (80 bytes)."""
    _fields_ = [("minv", C.c_double * 9), ("i", C.c_int32), ("j", C.c_int32)]


class SiftKeypoint(C.Structure):
    """``pano_sift_keypoint`` of include/pano360.h (32 bytes)."""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("size", C.c_float), ("angle", C.c_float),
                ("response", C.c_float), ("octave", C.c_int32), ("r", C.c_int32), ("c", C.c_int32)]


class Camera(C.Structure):
    """``pano_camera`` of include/pano360.h (120 bytes)."""
    _fields_ = [("proj", C.c_double * 9), ("frame", C.c_void_p),
                ("hat_x", C.c_void_p), ("hat_y", C.c_void_p),
                ("sh", C.c_int32), ("sw", C.c_int32),
                ("y0", C.c_int32), ("x0", C.c_int32), ("h", C.c_int32), ("w", C.c_int32)]


# every record of include/pano360.h by its C name
RECORDS = {
    "pano_patch": Patch, "pano_layout": Layout, "pano_camera": Camera, "pano_pair": Pair,
    "pano_sift_keypoint": SiftKeypoint, "pano_sift_args": SiftArgs, "pano_jpeg_image": JpegImage,
    "pano_view": View, "pano_view_mosaic": ViewMosaic, "pano_lens_frame": LensFrame,
    "pano_photo_frame": PhotoFrame, "pano_photo_pair": PhotoPair, "pano_photo_apply": PhotoApply,
    "pano_fuse_stack": FuseStack, "pano_fuse_params": FuseParams, "pano_align_stack": AlignStack,
    "pano_align_params": AlignParams, "pano_deghost_stack": DeghostStack,
    "pano_deghost_params": DeghostParams, "pano_flow_params": FlowParams, "pano_stitch_args": StitchArgs,
}

_vp, _i = C.c_void_p, C.c_int
_SIGNATURES = {
    "pano_version": (C.c_char_p, []),
    "pano_last_error": (C.c_char_p, []),
    "pano_device_count": (_i, []),
    "pano_pitch": (_i, [_i]),
    "pano_interior_block": (_i, []),
    "pano_ctx_create": (_i, [_i, _vp, C.POINTER(C.c_void_p)]),
    "pano_ctx_destroy": (_i, [_vp]),
    "pano_ctx_set_stream": (_i, [_vp, _vp]),
    "pano_ctx_set_option": (_i, [_vp, _i, _i]),
    "pano_ctx_get_option": (_i, [_vp, _i, C.POINTER(C.c_int)]),
    "pano_timing_enable": (_i, [_vp, _i]),
    "pano_kernel_count": (_i, []),
    "pano_kernel_name": (C.c_char_p, [_i]),
    "pano_timing_read": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "pano_add_weights": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "pano_warp_spherical": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i,
                                 _i, _vp, _vp, _vp, _vp]),
    "pano_warp_windows": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "pano_blur_tiles": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pano_ownership": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "pano_ownership_cameras": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "pano_owned_regions": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "pano_ownership_regions": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                    _i, _i, _vp, _vp]),
    "pano_multiband_blur": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, C.POINTER(C.c_int), _i,
                                 _vp, _vp]),
    "pano_multiband_blur_prepare": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pano_layout_windows": (_i, [_i, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "pano_layout_place": (_i, [_vp, _i, _vp, _vp, _vp]),
    "pano_interior_map": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "pano_interior_classes": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "pano_multiband_compose": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _i, _vp, _vp]),
    "pano_blend_cameras": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp,
                                _vp]),
    "pano_blur_tile_grid": (_i, [_vp]),
    "pano_overlap_blocks": (_i, [_i, _i]),
    "pano_overlap_stats": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pano_linear_blend": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "pano_no_blend": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "pano_median_cameras": (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.c_float, _vp, _vp, _vp, _vp, _i,
                                 _vp, _vp]),
    "pano_median_blend": (_i, [_vp, _vp, _i, _i, _i, C.c_float, _vp]),
    "pano_crop_rect": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "pano_blur_plane": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _i]),
    "pano_pyr_down": (_i, [_vp, _vp, _i, _i, _vp]),
    "pano_gray_u8": (_i, [_vp, _vp, _i, _i, _vp]),
    "pano_scale_step": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "pano_scale_space": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "pano_resize_up2": (_i, [_vp, _vp, _i, _i, _vp]),
    "pano_decimate2": (_i, [_vp, _vp, _i, _i, _vp]),
    "pano_subtract": (_i, [_vp, _vp, _vp, C.c_size_t, _vp]),
    "pano_pyr_down_image": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "pano_pyr_up_image": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _i]),
    "pano_u8_to_f32": (_i, [_vp, _vp, C.c_size_t, _vp]),
    "pano_laplacian_mix": (_i, [_vp, _vp, _vp, _vp, C.c_size_t, _i, _vp]),
    "pano_clip_u8": (_i, [_vp, _vp, C.c_size_t, _i, _vp]),
    "pano_poisson_blend": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, C.c_double, _i, _vp, _vp, _vp]),
    "pano_seam_levels": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "pano_seam_flood": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pano_seam_mask": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i]),
    "pano_alpha_blend": (_i, [_vp, _vp, _vp, _i, _vp, _i, C.c_int64, C.c_int64, C.c_int64, _i, _i,
                              _i, _vp]),
    "pano_seam_route_prepare": (_i, [_vp, _vp, _i, _i, _i, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp]),
    "pano_seam_route_flood": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "pano_seam_route": (_i, [_vp, _vp, _i, _i, _i, C.c_float, _vp, _vp, _vp]),
    "pano_flow_work_bytes": (C.c_size_t, [C.POINTER(Patch), _i, _i, _i, C.POINTER(FlowParams)]),
    "pano_flow_pyramid": (_i, [_vp, C.POINTER(Patch), _i, _i, _i, C.POINTER(FlowParams), _vp, C.c_int64]),
    "pano_flow_search": (_i, [_vp, C.POINTER(Patch), _i, _i, _i, C.POINTER(FlowParams), _vp, C.c_int64]),
    "pano_flow_smooth": (_i, [_vp, C.POINTER(Patch), _i, _i, _i, C.POINTER(FlowParams), _vp, C.c_int64]),
    "pano_flow_apply": (_i, [_vp, C.POINTER(Patch), _i, _i, _i, C.POINTER(FlowParams), _vp, C.c_int64, _vp, _vp]),
    "pano_flow_align": (_i, [_vp, C.POINTER(Patch), _i, _i, _i, C.POINTER(FlowParams), _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "pano_resize_u8": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i]),
    "pano_sift_extrema": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_float, C.c_float, C.c_float, _vp,
                               _vp, _i]),
    "pano_sift_orient": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i]),
    "pano_sift_describe": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "pano_sift_sort_work_bytes": (C.c_size_t, [_i]),
    "pano_sift_sort_unique": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "pano_knn2_work_bytes": (C.c_size_t, [_i, _i, _i]),
    "pano_knn2": (_i, [_vp, _vp, _i, _vp, _i, _i, C.c_float, _vp, _vp, _vp, _vp]),
    "pano_hom_ransac_work_bytes": (C.c_size_t, [_i, _i]),
    "pano_hom_ransac": (_i, [_vp, _vp, _vp, _vp, _i, _i, C.c_float, C.c_uint64, _vp, _vp, _vp, _vp,
                             _vp]),
    "pano_match_pack": (_i, [_vp, _vp, _vp, _i, C.c_double, _vp, _vp, _i, _vp, _vp, _vp]),
    "pano_ba_work_bytes": (C.c_size_t, [_i]),
    "pano_ba_residuals": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "pano_ba_normal": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp, C.c_double, _vp, _vp, _vp]),
    "pano_ba_refine": (_i, [_vp, _vp, C.c_int64, _vp, _i, _vp, _i, C.c_double, C.c_double,
                            C.c_double, _vp]),
    "pano_jpeg_decode": (_i, [_vp, _vp, _i, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64]),
    "pano_jpeg_encode_work_bytes": (C.c_size_t, [_i, _i, _i]),
    "pano_jpeg_encode": (_i, [_vp, _vp, _i, _i, C.c_int64, _i, _i, _vp, _vp, C.c_int64,
                             C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "pano_jpeg_encode_batch_work_bytes": (C.c_size_t, [C.c_int64, _i]),
    "pano_jpeg_encode_batch": (_i, [_vp, C.POINTER(JpegImage), _i, _i, _i, _vp, _vp, C.c_int64,
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "pano_png_filter": (_i, [_vp, _vp, _i, _i, C.c_int64, _i, _vp]),
    "pano_deflate_work_bytes": (C.c_size_t, [C.c_int64]),
    "pano_deflate": (_i, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(C.c_void_p),
                         C.POINTER(C.c_int64), C.POINTER(C.c_uint32)]),
    "pano_deflate_lengths": (_i, [_vp, _vp, _i, _i, _vp]),
    "pano_harris": (_i, [_vp, _vp, _i, _i, C.c_float, _vp]),
    "pano_sobel": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "pano_msop_smooth": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "pano_msop_candidates_work_bytes": (C.c_size_t, [_i, _i]),
    "pano_msop_candidates": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "pano_msop_cut_work_bytes": (C.c_size_t, [_i]),
    "pano_msop_cut": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "pano_ssc_probe_work_bytes": (C.c_size_t, [_i, _i]),
    "pano_ssc_probe": (_i, [_vp, _vp, _i, C.c_double, _i, _i, _i, _i, _vp, _vp, _vp]),
    "pano_msop_describe": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp,
                                _vp]),
    "pano_mip_u8": (_i, [_vp, _vp, _i, _i, C.c_int64, _vp, C.POINTER(C.c_int64), _i]),
    "pano_view_render": (_i, [_vp, _vp, C.POINTER(C.c_int64), _i, C.POINTER(ViewMosaic),
                              C.POINTER(View), _i]),
    "pano_fill_u8": (_i, [_vp, _vp, C.c_int64, _vp, C.c_int64, _i, _i, _i, _vp, C.c_int64]),
    "pano_select_u8": (_i, [_vp, _vp, _vp, _vp, _vp, C.c_int64]),
    "pano_lens_undistort_u8": (_i, [_vp, C.POINTER(LensFrame), _i]),
    "pano_photo_stats": (_i, [_vp, C.POINTER(PhotoFrame), _i, C.POINTER(PhotoPair), _i, _i, _i, _i,
                              C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, _vp]),
    "pano_photo_apply_u8": (_i, [_vp, C.POINTER(PhotoApply), _i]),
    "pano_fuse_work_bytes": (C.c_size_t, [_i, _i, _i]),
    "pano_fuse_u8": (_i, [_vp, C.POINTER(FuseStack), _i, C.POINTER(FuseParams), _vp, C.c_int64]),
    "pano_align_work_bytes": (C.c_size_t, [_i, _i, _i]),
    "pano_align_mtb": (_i, [_vp, C.POINTER(AlignStack), _i, C.POINTER(AlignParams), _vp, C.c_int64]),
    "pano_deghost_work_bytes": (C.c_size_t, [_i, _i, _i]),
    "pano_deghost_u8": (_i, [_vp, C.POINTER(DeghostStack), _i, C.POINTER(DeghostParams), _vp, C.c_int64]),
    "pano_sift_detect": (_i, [_vp, _vp]),
    "pano_sift_detect_replaying": (_i, [_vp]),
    "pano_stitch_multiband": (_i, [_vp, _vp, _i]),
    "pano_stitch_counts": (_i, [_vp, _vp, _vp]),
    "pano_stitch_verify": (_i, [_vp]),
}
EXPORTS = tuple(_SIGNATURES)
# the exports whose int result is a value, not a status: ``call`` refuses them (and whatever
# returns no int); they are called through ``lib()``
VALUE_RESULTS = frozenset((
    "pano_device_count", "pano_pitch", "pano_interior_block", "pano_kernel_count",
    "pano_blur_tile_grid", "pano_overlap_blocks", "pano_sift_detect_replaying"))


def sources_digest():
    """sha256 over everything the library is compiled from (csrc/*.hip, *.h, *.inc, the Makefile,
    include/pano360.h), names included.  A package installed without ../include hashes the rest."""
    import hashlib
    src = os.path.join(_HERE, "csrc")
    files = sorted(os.path.join(src, f) for f in os.listdir(src)
                   if f.endswith((".hip", ".h", ".inc")) or f == "Makefile")
    files.append(os.path.join(os.path.dirname(_HERE), "include", "pano360.h"))
    h = hashlib.sha256()
    for path in files:
        if not os.path.exists(path):
            continue
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as fid:
            h.update(fid.read())
    return h.hexdigest()


BUILD_RECORD = os.path.join(_HERE, "csrc", ".build_stamp")


def build(force=False):
    """Compile the HIP sources in-tree (hipcc cross-compiles without a GPU).  `make` alone trusts
    file times, which a checkout or a copied tree does not keep: the objects are therefore
    stamped with the digest of the sources they were built from, and a tree whose stamp is missing
    or differs is rebuilt from scratch (`make -B`).  The stamp says what happened
    (`csrc/.build_stamp`: digest, mode "full" | "incremental" | "up to date")."""
    import json
    src = os.path.join(_HERE, "csrc")
    digest = sources_digest()
    have = None
    try:
        with open(BUILD_RECORD) as fid:
            have = json.load(fid).get("sources_sha256")
    except (OSError, ValueError):
        pass
    full = force or have != digest or not os.path.exists(LIB_PATH)
    before = os.path.getmtime(LIB_PATH) if os.path.exists(LIB_PATH) else None
    cmd = ["make", "-C", src, "-s", "-j4"] + (["-B"] if full else [])
    subprocess.check_call(cmd)
    after = os.path.getmtime(LIB_PATH)
    mode = "full" if full else ("incremental" if after != before else "up to date")
    with open(BUILD_RECORD, "w") as fid:
        json.dump({"sources_sha256": digest, "mode": mode}, fid)
    return LIB_PATH


_lib = None


def lib():
    """Load (once) and return the bound library; raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PanoError(
                f"{LIB_PATH} is missing: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        import torch  # noqa: F401  (pins the HIP runtime, see module docstring)
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def _ptr(t):
    """A tensor's address as a ctypes argument (None stays a null pointer)."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _engine(eng):
    """``eng``, or the process's engine."""
    from . import engine
    return eng or engine.engine()


def is_u8(x):
    """Whether a host array or a tensor holds uint8."""
    return str(x.dtype) in ("uint8", "torch.uint8")


def is_rgb_u8(img):
    """Whether a host array or a tensor is uint8 [h][w][3], what ``rgb_on_device`` takes."""
    return is_u8(img) and len(img.shape) == 3 and img.shape[2] == 3


def rgb_on_device(img, eng):
    """A [h][w][3] host array or tensor as a tensor on ``eng``'s device whose pixels are 3 elements
    apart and whose rows are at least 3 w apart - what the native calls take with a row pitch.  A
    host array is uploaded (a read-only one is copied first: torch wraps writable memory only); a
    tensor is copied only when its strides are not like that, so a crop view of a dense image is
    returned as it is, the same object when it is on the device already."""
    import torch
    if not isinstance(img, torch.Tensor):
        img = np.ascontiguousarray(img)
        img = torch.from_numpy(img if img.flags.writeable else img.copy())
    img = img.to(torch.device(eng.device))
    if img.stride(2) != 1 or img.stride(1) != 3 or img.stride(0) < 3 * img.shape[1]:
        img = img.contiguous()
    return img


def check(status, what):
    if status != 0:
        msg = lib().pano_last_error().decode("utf-8", "replace")
        raise PanoError(f"{what} failed ({status}): {msg}")


def _pointer_kinds(name, fn):
    """Per argument of the status function ``fn``: None for a scalar, else the pointer type an
    address is handed over as (``c_void_p``, or the ``POINTER(T)`` / ``c_char_p`` it is cast to)."""
    if name in VALUE_RESULTS or fn.restype is not C.c_int:
        raise TypeError(f"{name} returns a value, not a status: call it through lib()")
    return tuple(t if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer) else None
                 for t in fn.argtypes)


_kinds = {}     # name -> (function, its _pointer_kinds)


def call(name, *args, via=None):
    """``lib().name(*args)`` with the status checked.  The function's argtypes decide what is
    converted: in a pointer position a tensor (or a view of one) and a NumPy array become their
    addresses, None stays a null pointer, and everything else - ctypes objects, ``byref``, plain
    integer addresses - is passed as it is; in a scalar position an array is refused.  Nothing
    here judges the memory behind an address (device, dtype, contiguity).  ``via``: the object
    whose attribute ``name`` is called with the converted arguments instead (an engine's ``lib``,
    which a caller may have wrapped); the declaration is ``lib()``'s either way."""
    fn = getattr(lib(), name)
    fn_kinds = _kinds.get(name)
    if fn_kinds is None or fn_kinds[0] is not fn:
        fn_kinds = _kinds[name] = (fn, _pointer_kinds(name, fn))
    kinds = fn_kinds[1]
    if len(args) != len(kinds):
        raise TypeError(f"{name} takes {len(kinds)} arguments, {len(args)} were given")
    args = list(args)
    for k, kind in enumerate(kinds):
        x = args[k]
        if x is None or type(x) is int or type(x) is float:
            continue
        tensor = hasattr(x, "data_ptr")
        if not tensor and not isinstance(x, np.ndarray):
            continue
        if kind is None:
            if x.ndim > 0:
                raise TypeError(f"{name}: argument {k} is a scalar, an array was given")
            continue
        address = C.c_void_p(x.data_ptr() if tensor else x.ctypes.data)
        args[k] = address if kind is C.c_void_p else C.cast(address, kind)
    check((fn if via is None else getattr(via, name))(*args), name)
