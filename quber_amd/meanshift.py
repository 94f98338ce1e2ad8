"""Options of the mean-shift clustering that turns a UCN embedding map into initial masks (csrc/meanshift.hip; INTEGRATION.md
"Initial masks from pixel embeddings"): the reference's ``clustering_features`` -> ``mean_shift_smart_init`` and ``filter_labels_depth``
(eval/base_model.py:622-840, :34-47), cosine metric.  Plain host-side data, like ``masknms.MaskNMS``: the work is done by
``Engine.meanshift`` and its stage entries."""
import numbers

import numpy as np

CHANNELS = 64                      # csrc/meanshift.hip: MS_C (every UCN config of the reference has NUM_UNITS: 64)
MAX_SEEDS = 128                    # csrc/meanshift.hip: MS_SMAX
UCN_DEPTH_THRESHOLD = {"OSD": 0.8, "OCID": 0.5, "HOPE": 0.5, "DoPose": 0.5}      # eval/base_model.py:598-601


def _number(name, v, lo, hi, integer=False):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral if integer else numbers.Real):
        raise ValueError(f"cluster: {name} must be {'an integer' if integer else 'a number'}")
    v = int(v) if integer else float(v)
    if not (np.isfinite(v) and lo <= v <= hi):
        raise ValueError(f"cluster: {name} must lie in {lo} .. {hi}")
    return v


class MeanShift:
    """num_seeds: seeds picked farthest-first (the reference's 100; <= 128).  kappa: concentration of the von Mises-Fisher kernel (20).
    iters: hill-climbing rounds, a fixed count (10).  alpha: the embedding margin; seeds within epsilon = 2 alpha (cosine distance) of
    one another share a label (0.02 in every UCN yaml).  depth_threshold: None, or the share of a mask's pixels that must have depth
    z > 0 for the mask to stay (``filter_labels_depth``).  seed: of the RandomState the first seed of every frame is drawn from.

    The object OWNS that stream: it is the one mutable thing in it, and it is not part of ``==`` / ``hash`` (two objects with equal
    options are equal wherever their streams stand).  Every frame a predictor clusters takes one draw, so one object handed to two
    predictors interleaves their draws - give each predictor its own ``MeanShift`` where the first seeds must be reproducible per
    predictor.  ``reseed()`` rewinds the stream.  A call that raises before anything is launched has drawn nothing."""

    __slots__ = ("num_seeds", "kappa", "iters", "alpha", "depth_threshold", "seed", "_rng")

    def __init__(self, num_seeds=100, kappa=20.0, iters=10, alpha=0.02, depth_threshold=None, seed=0):
        self.num_seeds = _number("num_seeds", num_seeds, 1, MAX_SEEDS, integer=True)
        self.kappa = _number("kappa", kappa, 0.0, 64.0)      # exp(kappa) summed over 2^24 pixels stays inside float32
        self.iters = _number("iters", iters, 0, 1000, integer=True)
        self.alpha = _number("alpha", alpha, 0.0, 0.5)
        self.depth_threshold = None if depth_threshold is None else _number("depth_threshold", depth_threshold, 0.0, 1.0)
        self.seed = _number("seed", seed, 0, 2 ** 32 - 1, integer=True)
        self._rng = np.random.RandomState(self.seed)

    @classmethod
    def parse(cls, value):
        """None | MeanShift -> None | MeanShift."""
        if value is None or isinstance(value, cls):
            return value
        raise ValueError(f"cluster={value!r}: expected None or a quber_amd.meanshift.MeanShift")

    @classmethod
    def ucn(cls, dataset=None, **kw):
        """The reference's settings for `dataset`: the depth filter at 0.8 for OSD, 0.5 for OCID / HOPE / DoPose, none otherwise."""
        return cls(depth_threshold=UCN_DEPTH_THRESHOLD.get(dataset), **kw)

    @property
    def epsilon(self):
        return 2 * self.alpha

    def first_seeds(self, frames, n):
        """The first seed of each of `frames` frames of n pixels: one draw per frame, in frame order, from this object's
        RandomState(seed) - the reference's ``np.random.randint(0, n)`` (base_model.py:701) on a stream of its own."""
        return np.array([self._rng.randint(0, n) for _ in range(frames)], np.int32)

    def reseed(self):
        self._rng = np.random.RandomState(self.seed)

    def args(self):
        return self.num_seeds, self.kappa, self.iters, self.alpha, self.depth_threshold, self.seed

    def __eq__(self, other):
        return isinstance(other, MeanShift) and self.args() == other.args()

    def __hash__(self):
        return hash(self.args())

    def __repr__(self):
        return "MeanShift(num_seeds=%r, kappa=%r, iters=%r, alpha=%r, depth_threshold=%r, seed=%r)" % self.args()
