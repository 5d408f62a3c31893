"""``features.matching`` of the reference (features.py:235-320) - detection, 2-NN matching, the
ratio test and a RANSAC homography for every pair - and its command line, served by the MI355X
build: ``python features.py --path DIR`` writes ``matches_<DIR>.npz``
(``--detector msop``: the MSOP detector of features.py:27-156, ``matches_<DIR>_msop.npz``)."""
import logging

from pano360_amd.features import (DSIZE, N_MIN_MATCH, RANSAC, _match_hom, _reverse,  # noqa: F401
                                  find_homography, flann_matching, main, matching, msop_detect,
                                  msop_detector, rot_mat, sift_detector, ssc)

if __name__ == "__main__":
    logging.basicConfig(level=logging.DEBUG)
    main()
