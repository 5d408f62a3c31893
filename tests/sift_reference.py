"""Two SIFT detections of one frame compared: what differs between two runs of the HIP detector on
the same frame and what does not.  Keypoints - position, size, response, octave, the extremum's row
and column - bit for bit; angles to 0.01 degrees and descriptors to 2 (of 0 .. 255) in under 2 % of
their entries: both are sums of LDS atomics, whose order changes from run to run."""
import numpy as np


def assert_same_detection(kps, desc, kps_ref, desc_ref):
    """``kps`` / ``kps_ref``: KP_DTYPE arrays; ``desc`` / ``desc_ref``: [K][128] float32, on the
    device or the host."""
    desc = desc.cpu().numpy() if hasattr(desc, "cpu") else np.asarray(desc)
    desc_ref = desc_ref.cpu().numpy() if hasattr(desc_ref, "cpu") else np.asarray(desc_ref)
    assert len(kps) == len(kps_ref)
    assert desc.shape == desc_ref.shape == (len(kps_ref), 128)
    for key in ("x", "y", "size", "response", "octave", "r", "c"):
        assert np.array_equal(kps[key], kps_ref[key]), key
    if len(kps_ref) == 0:
        return
    dang = np.abs(kps["angle"] - kps_ref["angle"])
    assert np.minimum(dang, 360 - dang).max() <= 0.01
    diff = np.abs(desc - desc_ref)
    assert diff.max() <= 2 and (diff > 0).mean() < 0.02
