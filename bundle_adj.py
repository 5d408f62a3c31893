"""Module path ``bundle_adj``: the reference module's surface (bundle_adj.py), so camera
caches move between the reference CLI and this build and ``traverse`` is where the reference
has it."""
from pano360_amd.bundle_adj import (  # noqa: F401
    LM_LAMBDA, LM_MAX_ITER, MIN_MATCH_ERROR, PARAMS_PER_CAMERA, TERMS_PER_MATCH, Image,
    IncrementalBundleAdjuster, Refinement, camera_to_params, dr_dvi, get_diff, get_focal,
    intrinsics, loss, mat_to_angle, params_to_camera, refine, residuals, rotation_to_mat,
    straighten, to_rotation, traverse)
