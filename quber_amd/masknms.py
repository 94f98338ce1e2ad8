"""Options of the mask NMS that makes scored, overlapping initial masks disjoint (csrc/masknms.hip; INTEGRATION.md "Overlapping
initial masks"): the reference's ``nms`` + ``combine_masks_with_NMS`` (eval/refiner_model.py:683-740, eval/base_model.py:1027-1086,
1154-1190).  Plain host-side data, like ``cleanup.Cleanup``: the work is done by ``Engine.mask_nms``."""
import numbers

import numpy as np

ON_TOP = ("large", "small")        # the C ABI's on_top = 0, 1
MAX_MASKS = 1024                   # csrc/masknms.hip: MN_MAX


class MaskNMS:
    """thresh: a mask is suppressed by a kept, higher-scored one when their IoU (float32) exceeds it - the reference's 0.7.
    on_top: which survivors end up on top where survivors overlap - "large" (the reference: painted in order of area, the largest
    last) or "small" (the reverse order: an object inside a larger proposal stays visible)."""

    __slots__ = ("thresh", "on_top")

    def __init__(self, thresh=0.7, on_top="large"):
        if isinstance(thresh, (bool, np.bool_)) or not isinstance(thresh, numbers.Real):
            raise ValueError("nms: thresh must be a number")
        thresh = float(thresh)
        if not (np.isfinite(thresh) and 0.0 <= thresh <= 1.0):
            raise ValueError("nms: thresh must lie in 0 .. 1")
        if on_top not in ON_TOP:
            raise ValueError(f"nms: on_top={on_top!r}: expected 'large' or 'small'")
        self.thresh, self.on_top = thresh, on_top

    @classmethod
    def parse(cls, value):
        """None | MaskNMS -> None | MaskNMS."""
        if value is None or isinstance(value, cls):
            return value
        raise ValueError(f"nms={value!r}: expected None or a quber_amd.masknms.MaskNMS")

    def args(self):
        """The two option arguments of the C ABI: thresh (rounded to float32 there), on_top."""
        return self.thresh, ON_TOP.index(self.on_top)

    def __eq__(self, other):
        return isinstance(other, MaskNMS) and self.args() == other.args()

    def __hash__(self):
        return hash(self.args())

    def __repr__(self):
        return "MaskNMS(thresh=%r, on_top=%r)" % (self.thresh, self.on_top)


def check_scores(scores, n, what="mask_scores"):
    """The scores of n masks as a contiguous float32 [n] array; ValueError when they are missing, of another length or not finite."""
    if scores is None and n == 0:
        return np.zeros((0,), np.float32)
    if scores is None:
        raise ValueError(f"nms: {what} is required when nms= is set")
    s = np.asarray(scores)
    if s.dtype == np.bool_ or not (np.issubdtype(s.dtype, np.floating) or np.issubdtype(s.dtype, np.integer)):
        raise ValueError(f"nms: {what} must be numbers")
    if s.shape != (n,):
        raise ValueError(f"nms: {what} of shape {s.shape} for {n} masks")
    with np.errstate(over="ignore"):                 # (a float64 beyond float32's range becomes inf, and is refused below)
        s = np.ascontiguousarray(s, dtype=np.float32)
    if not np.isfinite(s).all():
        raise ValueError(f"nms: {what} must be finite")
    return s
