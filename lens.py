"""Lens correction at the ingest, served by the MI355X build: ``LensModel``, ``load``,
``fit_focal``, ``undistort_device`` and ``undistort`` of ``pano360_amd.lens`` (the reference has
no lens code: it assumes an ideal pinhole camera)."""
from pano360_amd.lens import (Calibration, LensModel, fit_focal, load,  # noqa: F401
                              undistort, undistort_device)
