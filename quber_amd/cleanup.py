"""Options of the connected-component clean-up of the refined instances (csrc/cleanup.hip; INTEGRATION.md "Connected-component
clean-up").  Plain host-side data: the work is done by ``Engine.cleanup_ids`` / ``Engine.cleanup_post``."""
import numbers

import numpy as np


class Cleanup:
    """keep_largest: every instance keeps its largest ``connectivity``-connected component only; otherwise components smaller than
    ``min_island_area`` pixels are dropped (the largest always stays).  ``max_hole_area`` > 0: a void region of fewer pixels whose
    neighbours all belong to one instance is given to it."""

    __slots__ = ("keep_largest", "connectivity", "min_island_area", "max_hole_area")

    def __init__(self, keep_largest=False, connectivity=8, min_island_area=0, max_hole_area=0):
        def integer(name, v):                      # Python and numpy integers; no bool, no float
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral):
                raise ValueError(f"cleanup: {name} must be an integer")
            return int(v)
        if not isinstance(keep_largest, (bool, np.bool_)) and not (isinstance(keep_largest, numbers.Integral) and keep_largest in (0, 1)):
            raise ValueError("cleanup: keep_largest must be a bool")
        connectivity = integer("connectivity", connectivity)
        if connectivity not in (4, 8):
            raise ValueError("cleanup: connectivity must be 4 or 8")
        min_island_area, max_hole_area = integer("min_island_area", min_island_area), integer("max_hole_area", max_hole_area)
        if not (0 <= min_island_area < 2 ** 31 and 0 <= max_hole_area < 2 ** 31):
            raise ValueError("cleanup: the areas must lie in 0 .. 2^31 - 1")
        self.keep_largest, self.connectivity = bool(keep_largest), int(connectivity)
        self.min_island_area, self.max_hole_area = int(min_island_area), int(max_hole_area)

    @classmethod
    def uois(cls):
        """largest_connected_component(mask, connectivity=4) of the reference's UOIS / RICE path (eval/utilities.py:726-748)."""
        return cls(keep_largest=True, connectivity=4)

    @classmethod
    def sam(cls, area=300):
        """remove_small_regions(mask, area, "holes") of the reference's SAM refiner (eval/refiner_model.py:526-549, 774)."""
        return cls(connectivity=8, max_hole_area=area)

    @classmethod
    def parse(cls, value):
        """None | Cleanup | "largest" (= uois()) | "holes" (= sam()) -> None | Cleanup."""
        if value is None or isinstance(value, cls):
            return value
        if value == "largest":
            return cls.uois()
        if value == "holes":
            return cls.sam()
        raise ValueError(f"cleanup={value!r}: expected None, a Cleanup, 'largest' or 'holes'")

    def args(self):
        """The four trailing option arguments of the C ABI."""
        return self.connectivity, int(self.keep_largest), self.min_island_area, self.max_hole_area

    def __eq__(self, other):
        return isinstance(other, Cleanup) and self.args() == other.args()

    def __hash__(self):
        return hash(self.args())

    def __repr__(self):
        return "Cleanup(keep_largest=%r, connectivity=%d, min_island_area=%d, max_hole_area=%d)" % (
            self.keep_largest, self.connectivity, self.min_island_area, self.max_hole_area)
