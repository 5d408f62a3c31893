"""``blend.laplacian_blending`` (blend.py:105-140), ``blend.poisson_blend`` (blend.py:175-203),
``blend.graph_cut`` (blend.py:56-100) and ``blend.alpha_blend`` (blend.py:48-53) of the reference,
served by the MI355X build.  ``poisson_matrix`` returns a SciPy sparse matrix and is not provided
(the product does not depend on SciPy); ``warp`` is out of scope (its ``cv2.remap`` leaves the
pixels outside the source undefined; the stitcher's own spherical warp covers the use)."""
from pano360_amd.blend import (alpha_blend, graph_cut, laplacian_blending,  # noqa: F401
                               poisson_blend)
