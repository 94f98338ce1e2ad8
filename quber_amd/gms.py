"""Options of the Gaussian mean shift that turns UOIS-Net-3D's centre votes into initial masks, and of the initial mask processing (IMP)
that follows it (csrc/gms.hip; INTEGRATION.md "Initial masks from centre votes"): the reference's ``DSNWrapper.cluster`` ->
``GaussianMeanShift.mean_shift_smart_init`` (uois/src/segmentation.py:129-187, uois/src/cluster.py) and
``UOISNet3D.process_initial_masks`` (segmentation.py:425-491).  Plain host-side data, like ``meanshift.MeanShift``: the work is done by
``Engine.gms`` and its stage entries."""
import numpy as np

from .meanshift import _number

MAX_SEEDS = 256                    # csrc/gms.hip: GM_SMAX
MAX_KSIZE = 15                     # csrc/gms.hip: GM_KMAX
IMP_LDS_BYTES = 152 * 1024         # csrc/gms.hip: GM_LDS_MAX, what the IMP's two bit planes may take


def imp_plane_bytes(h, w):
    """The LDS the IMP needs for a frame: two bit planes of h x ceil(w / 32) words."""
    return 2 * int(h) * ((int(w) + 31) // 32) * 4


class IMP:
    """ksize: the side of OpenCV's elliptic structuring element every mask is opened, then closed with (the reference's 9; odd, 1..15).
    largest: keep the largest 4-connected component of every mask afterwards (True in the reference)."""

    __slots__ = ("ksize", "largest")

    def __init__(self, ksize=9, largest=True):
        self.ksize = _number("imp ksize", ksize, 1, MAX_KSIZE, integer=True)
        if self.ksize % 2 == 0:
            raise ValueError("cluster: imp ksize must be odd")
        if not isinstance(largest, (bool, np.bool_)):
            raise ValueError("cluster: imp largest must be a bool")
        self.largest = bool(largest)

    @classmethod
    def parse(cls, value):
        """None | IMP -> None | IMP."""
        if value is None or isinstance(value, cls):
            return value
        raise ValueError(f"imp={value!r}: expected None or a quber_amd.gms.IMP")

    def args(self):
        return self.ksize, self.largest

    def __eq__(self, other):
        return isinstance(other, IMP) and self.args() == other.args()

    def __hash__(self):
        return hash(self.args())

    def __repr__(self):
        return "IMP(ksize=%r, largest=%r)" % self.args()


_DEFAULT_IMP = object()


class GaussianMeanShift:
    """num_seeds: seeds drawn with probability proportional to the distance from the seeds already chosen (the reference's 200; <= 256).
    sigma: bandwidth of the Gaussian kernel, in the votes' unit (0.02 m).  iters: hill-climbing rounds, a fixed count (10).  epsilon:
    seeds within this euclidean distance of one another share a label (0.05).  subsample: every subsample-th foreground pixel seeds and
    climbs (5); all of them are assigned.  min_pixels: clusters with fewer pixels are dropped (300).  imp: an ``IMP`` or None (no
    processing); the default is the reference's IMP(9, True).  seed: of the RandomState the first seed and the 32-bit draws of every
    frame come from.

    The object OWNS that stream, exactly as ``MeanShift`` does: it is not part of ``==`` / ``hash``, every frame a predictor clusters
    takes ``num_seeds`` draws (the first seed, then one 32-bit draw per further seed), one object handed to two predictors interleaves
    their draws, ``reseed()`` rewinds the stream, and a call that raises before anything is launched has drawn nothing."""

    __slots__ = ("num_seeds", "sigma", "iters", "epsilon", "subsample", "min_pixels", "imp", "seed", "_rng")

    def __init__(self, num_seeds=200, sigma=0.02, iters=10, epsilon=0.05, subsample=5, min_pixels=300, imp=_DEFAULT_IMP, seed=0):
        self.num_seeds = _number("num_seeds", num_seeds, 1, MAX_SEEDS, integer=True)
        self.sigma = _number("sigma", sigma, 1e-6, 1e6)
        self.iters = _number("iters", iters, 0, 1000, integer=True)
        self.epsilon = _number("epsilon", epsilon, 0.0, 1e6)
        self.subsample = _number("subsample", subsample, 1, 64, integer=True)
        self.min_pixels = _number("min_pixels", min_pixels, 0, 2 ** 24, integer=True)
        self.imp = IMP() if imp is _DEFAULT_IMP else IMP.parse(imp)
        self.seed = _number("seed", seed, 0, 2 ** 32 - 1, integer=True)
        self._rng = np.random.RandomState(self.seed)

    @classmethod
    def parse(cls, value):
        """None | GaussianMeanShift -> None | GaussianMeanShift."""
        if value is None or isinstance(value, cls):
            return value
        raise ValueError(f"cluster={value!r}: expected None or a quber_amd.gms.GaussianMeanShift")

    @classmethod
    def uois(cls, **kw):
        """The values of the reference's ext_modules/uois/uoisnet3d.yaml (they are the defaults; spelled out so that they stay)."""
        return cls(**dict(dict(num_seeds=200, sigma=0.02, iters=10, epsilon=0.05, subsample=5, min_pixels=300, imp=IMP(9, True)), **kw))

    def n_sub(self, n):
        """The points that seed and climb, of n foreground pixels."""
        return -(-int(n) // self.subsample)

    def draws(self, n_subs):
        """Per frame, in frame order, from this object's RandomState(seed): the first seed, ``randint(0, max(n_sub, 1))``, then
        num_seeds - 1 32-bit draws r_k.  n_subs: the n_sub of every frame -> (first i32 [B], draws u32 [B, num_seeds]; column 0 is 0)."""
        first = np.zeros(len(n_subs), np.int32)
        r = np.zeros((len(n_subs), self.num_seeds), np.uint32)
        for b, ns in enumerate(n_subs):
            first[b] = self._rng.randint(0, max(int(ns), 1))
            r[b, 1:] = self._rng.randint(0, 2 ** 32, size=self.num_seeds - 1, dtype=np.uint64).astype(np.uint32)
        return first, r

    def reseed(self):
        self._rng = np.random.RandomState(self.seed)

    def args(self):
        return self.num_seeds, self.sigma, self.iters, self.epsilon, self.subsample, self.min_pixels, self.imp, self.seed

    def __eq__(self, other):
        return isinstance(other, GaussianMeanShift) and self.args() == other.args()

    def __hash__(self):
        return hash(self.args())

    def __repr__(self):
        return "GaussianMeanShift(num_seeds=%r, sigma=%r, iters=%r, epsilon=%r, subsample=%r, min_pixels=%r, imp=%r, seed=%r)" % self.args()
