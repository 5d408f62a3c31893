"""Local alignment of overlapping frames before the blend, served by the MI355X build:
``FlowParams``, ``pairs_for``, ``fields_device`` and ``align_device`` of ``pano360_amd.flow`` (the
reference blends the frames as they are registered)."""
from pano360_amd.flow import (FlowParams, align_device, fields_device,  # noqa: F401
                              pairs_for)
