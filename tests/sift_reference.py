"""Two SIFT detections of one frame compared: two runs of the HIP detector on the same frame agree
bit for bit - keypoints (position, size, angle, response, octave, the extremum's row and column) and
descriptors.  The lists are filled by atomics in an order that changes from run to run, but nothing
that is kept depends on it: the orientation and descriptor histograms are sums of integer
fixed-point votes (sift.hip), which do not depend on the order of the additions, and the sort
(sift_sort.hip) is stable and drops keypoints that tie on all of its keys as duplicates."""
import numpy as np


def assert_same_detection(kps, desc, kps_ref, desc_ref):
    """``kps`` / ``kps_ref``: KP_DTYPE arrays; ``desc`` / ``desc_ref``: [K][128] float32, on the
    device or the host."""
    desc = desc.cpu().numpy() if hasattr(desc, "cpu") else np.asarray(desc)
    desc_ref = desc_ref.cpu().numpy() if hasattr(desc_ref, "cpu") else np.asarray(desc_ref)
    assert len(kps) == len(kps_ref)
    assert desc.shape == desc_ref.shape == (len(kps_ref), 128)
    for key in ("x", "y", "size", "angle", "response", "octave", "r", "c"):
        assert np.array_equal(kps[key], kps_ref[key]), key
    assert np.array_equal(desc, desc_ref), "descriptors differ"
