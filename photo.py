"""Photometric alignment of the frames before the stitch, served by the MI355X build:
``pair_table``, ``stats_device``, ``default_step``, ``solve``, ``estimate_device``,
``apply_device`` and ``correct_regions`` of ``pano360_amd.photo`` (the reference has one scalar
gain per camera, ``equalize_gains``)."""
from pano360_amd.photo import (PhotoModel, apply_device, correct_regions,  # noqa: F401
                               default_step, estimate_device, pair_table, solve, stats_device,
                               tables)
