"""``blend.laplacian_blending`` (blend.py:105-140) and ``blend.poisson_blend``
(blend.py:175-203) of the reference, served by the MI355X build.  ``poisson_matrix`` returns a
SciPy sparse matrix and is not provided (the product does not depend on SciPy); the other
experiments of the reference's blend.py (``warp``, ``graph_cut``, ``alpha_blend``) are out of
scope."""
from pano360_amd.blend import laplacian_blending, poisson_blend  # noqa: F401
