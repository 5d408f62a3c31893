"""Alignment of hand-held exposure brackets before they are fused, served by the MI355X build:
``AlignParams``, ``levels_for``, ``shifts_device``, ``align_device`` and ``align`` of
``pano360_amd.align`` (the reference reads one image per position)."""
from pano360_amd.align import (AlignParams, align, align_device, levels_for,  # noqa: F401
                               reach_for, shifts_device)
