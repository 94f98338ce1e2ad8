"""Options of the zoom-in refinement (csrc/zoom.hip; INTEGRATION.md "Zoom-in refinement"): the second, zoomed-in pass of the reference's
base models (``crop_rois`` / ``match_label_crop``, eval/base_model.py:843-961) - every first-pass instance is cropped with a padded box,
resized to a fixed square, refined again, and the crop results that agree with the mask they came from are painted back, far objects
first.  Plain host-side data, like ``masknms.MaskNMS``: the work is done by ``Engine.zoom_rois`` / ``zoom_crop`` / ``zoom_paste`` and
``RefinerModel``."""
import numbers

import numpy as np

MAX_CROP = 512                     # csrc/zoom.hip: the 32-bit bilinear sums and the float32 overlap ratio are exact up to 512 x 512 crops
MAX_IDS = 254                      # ids of a compact map


def _number(value, what):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, numbers.Real) or not np.isfinite(float(value)):
        raise ValueError(f"zoom: {what} must be a finite number")
    return value


class ZoomIn:
    """crop: edge of the square every instance is resized to (the reference's TRAIN.SYN_CROP_SIZE, 224); the network must accept a
    crop x crop frame.  padding: the box grows by rint(extent * padding) on every side (the reference's 0.25).  min_overlap: a crop-pass
    instance is kept when at least this share of it lies inside the mask its crop came from (the reference's 0.5).  batch: crops per
    call of the crop pass."""

    __slots__ = ("crop", "padding", "min_overlap", "batch")

    def __init__(self, crop=224, padding=0.25, min_overlap=0.5, batch=16):
        for v, what in ((crop, "crop"), (batch, "batch")):
            if _number(v, what) != int(v):
                raise ValueError(f"zoom: {what} must be an integer")
        crop, batch = int(crop), int(batch)
        if crop > MAX_CROP:
            raise ValueError(f"zoom: crop={crop} exceeds {MAX_CROP}: the exact integer and float32 arithmetic of the kernels rests on it")
        if crop < 16:
            raise ValueError("zoom: crop must be at least 16 (the network's smallest frame)")
        if batch < 1:
            raise ValueError("zoom: batch must be at least 1")
        padding, min_overlap = float(_number(padding, "padding")), float(_number(min_overlap, "min_overlap"))
        if not 0.0 <= padding <= 16.0:
            raise ValueError("zoom: padding must lie in 0 .. 16")
        if not 0.0 <= min_overlap <= 1.0:
            raise ValueError("zoom: min_overlap must lie in 0 .. 1")
        from . import engine as qengine
        qengine.make_config(crop, crop, max_batch=1, max_instances=64)       # (the frame the crop engine is configured for)
        self.crop, self.padding, self.min_overlap, self.batch = crop, padding, min_overlap, batch

    @classmethod
    def parse(cls, value):
        """None | ZoomIn -> None | ZoomIn."""
        if value is None or isinstance(value, cls):
            return value
        raise ValueError(f"zoom={value!r}: expected None or a quber_amd.zoom.ZoomIn")

    def args(self):
        return self.crop, self.padding, self.min_overlap, self.batch

    def __eq__(self, other):
        return isinstance(other, ZoomIn) and self.args() == other.args()

    def __hash__(self):
        return hash(self.args())

    def __repr__(self):
        return "ZoomIn(crop=%r, padding=%r, min_overlap=%r, batch=%r)" % self.args()
