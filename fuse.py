"""Exposure fusion of bracketed frames at the ingest, served by the MI355X build: ``FuseParams``,
``levels_for``, ``fuse_device``, ``fuse``, ``group_files`` and ``Bracket`` of ``pano360_amd.fuse``
(the reference takes one image per position)."""
from pano360_amd.fuse import (Bracket, FuseParams, fuse, fuse_device,  # noqa: F401
                              group_files, levels_for)
