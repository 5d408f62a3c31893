"""Deghosting of exposure brackets before they are fused, served by the MI355X build:
``DeghostParams``, ``masks_device``, ``deghost_device`` and ``deghost`` of ``pano360_amd.deghost``
(the reference reads one image per position)."""
from pano360_amd.deghost import (DeghostParams, deghost, deghost_device,  # noqa: F401
                                 masks_device)
