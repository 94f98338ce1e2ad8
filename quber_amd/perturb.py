"""Perturbed initial masks (csrc/perturb.hip; INTEGRATION.md "Perturbed initial masks"): the reference's ``perturb_seg``
(tools/ours/perturbation_utils.py:39-71) split into the part that draws random numbers - here, on the host - and the part that touches
pixels - ``Engine.perturb_masks``, on the device.  Plain host-side data, like ``cleanup.Cleanup``."""
import numbers

import numpy as np

OPS_PER_ROUND = 4          # perturbation_utils.py:52
COLUMNS = ("lx", "ly", "lw", "lh", "clear", "dilate", "size", "choice")


def perturb_program(h, w, rng, rounds=250, min_size=3, max_size=10):
    """The random walk ``perturb_seg`` takes on an h x w mask, drawn up front: int32 [4 * rounds, 8] with the rows
    (lx, ly, lw, lh, clear, dilate, size, choice).  ``rng`` is a ``numpy.random.RandomState``; per operation the draws are, in the
    reference's order (perturbation_utils.py:53-66, 23 / 29, 11),

        1. lx = randint(w)              3. lw = randint(lx + 1, w + 1)      5. clear  = rand() < 0.25      7. size   = randint(min_size, max_size)
        2. ly = randint(h)              4. lh = randint(ly + 1, h + 1)      6. dilate = rand() < 0.5       8. choice = randint(1, 5)

    four operations per round.  How many numbers an operation draws does not depend on the mask, so with ``RandomState(s)`` this is
    the stream ``np.random.seed(s); perturb_seg(gt, t)`` consumes - up to the round at which that call stops."""
    prog = np.empty((OPS_PER_ROUND * rounds, 8), np.int32)
    for k in range(OPS_PER_ROUND * rounds):
        lx = rng.randint(w)
        ly = rng.randint(h)
        lw = rng.randint(lx + 1, w + 1)
        lh = rng.randint(ly + 1, h + 1)
        clear = rng.rand() < 0.25
        dilate = rng.rand() < 0.5
        size = rng.randint(min_size, max_size)
        choice = rng.randint(1, 5)
        prog[k] = (lx, ly, lw, lh, clear, dilate, size, choice)
    return prog


class Perturb:
    """iou_target: the IoU with the uploaded mask below which a mask's walk stops - a float, or an array that broadcasts to the
    [frames, masks] of a call (per-mask targets).  Mask i of frame b of a call with N masks per frame walks the program of
    ``RandomState(seed + b * N + i)``; ``seeds``: an array that broadcasts to [frames, masks] instead.  rounds / min_size / max_size:
    perturb_seg's 250 rounds and random_dilate / random_erode's sizes randint(3, 10)."""

    __slots__ = ("iou_target", "seed", "seeds", "rounds", "min_size", "max_size", "_cache")

    def __init__(self, iou_target, seed=0, rounds=250, min_size=3, max_size=10, seeds=None):
        def integer(name, v):                      # Python and numpy integers; no bool, no float
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral):
                raise ValueError(f"perturb: {name} must be an integer")
            return int(v)
        t = np.asarray(iou_target)
        if t.dtype == np.bool_ or not (np.issubdtype(t.dtype, np.floating) or np.issubdtype(t.dtype, np.integer)) or t.ndim > 2 or t.size == 0:
            raise ValueError("perturb: iou_target must be a number or an array of at most two dimensions")
        t = t.astype(np.float64)
        if not (np.isfinite(t).all() and (t >= 0.0).all() and (t <= 1.0).all()):
            raise ValueError("perturb: iou_target must lie in 0 .. 1")
        seed, rounds = integer("seed", seed), integer("rounds", rounds)
        min_size, max_size = integer("min_size", min_size), integer("max_size", max_size)
        if not 0 <= seed < 2 ** 31:
            raise ValueError("perturb: seed must lie in 0 .. 2^31 - 1")
        if not 1 <= rounds <= 100000:
            raise ValueError("perturb: rounds must lie in 1 .. 100000")
        if not 1 <= min_size < max_size <= 16:     # sizes are drawn from [min_size, max_size): the kernel holds elements up to 15 x 15
            raise ValueError("perturb: sizes need 1 <= min_size < max_size <= 16")
        if seeds is not None:
            s = np.asarray(seeds)
            if s.dtype == np.bool_ or not np.issubdtype(s.dtype, np.integer) or s.ndim > 2 or s.size == 0 or (s < 0).any() or (s >= 2 ** 32).any():
                raise ValueError("perturb: seeds must be integers in 0 .. 2^32 - 1, at most two dimensions")
            seeds = s.astype(np.int64)
        self.iou_target, self.seed, self.seeds = t, seed, seeds
        self.rounds, self.min_size, self.max_size = rounds, min_size, max_size
        self._cache = {}

    @property
    def n_ops(self):
        return OPS_PER_ROUND * self.rounds

    def targets(self, frames, masks):
        """float64 [frames, masks]."""
        try:
            return np.ascontiguousarray(np.broadcast_to(self.iou_target, (frames, masks)))
        except ValueError:
            raise ValueError(f"perturb: iou_target of shape {self.iou_target.shape} does not broadcast to {(frames, masks)}") from None

    def mask_seeds(self, frames, masks):
        """int64 [frames, masks]: seed + b * masks + i, or the explicit seeds."""
        if self.seeds is None:
            return self.seed + np.arange(frames * masks, dtype=np.int64).reshape(frames, masks)
        try:
            return np.ascontiguousarray(np.broadcast_to(self.seeds, (frames, masks)))
        except ValueError:
            raise ValueError(f"perturb: seeds of shape {self.seeds.shape} do not broadcast to {(frames, masks)}") from None

    def programs(self, frames, masks, h, w):
        """int32 [frames, masks, 4 * rounds, 8].  A pure function of the arguments and the options, so the result is kept: a predictor
        that perturbs frame after frame draws its programs once per (frames, masks, h, w)."""
        key = (frames, masks, h, w)
        if key not in self._cache:
            if len(self._cache) >= 8:
                self._cache.pop(next(iter(self._cache)))
            seeds = self.mask_seeds(frames, masks)
            out = np.empty((frames, masks, self.n_ops, 8), np.int32)
            for b in range(frames):
                for i in range(masks):
                    out[b, i] = perturb_program(h, w, np.random.RandomState(int(seeds[b, i])), self.rounds, self.min_size, self.max_size)
            out.setflags(write=False)
            self._cache[key] = out
        return self._cache[key]

    def _key(self):
        return (self.iou_target.shape, self.iou_target.tobytes(), self.seed, None if self.seeds is None else (self.seeds.shape, self.seeds.tobytes()),
                self.rounds, self.min_size, self.max_size)

    def __eq__(self, other):
        return isinstance(other, Perturb) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        t = float(self.iou_target) if self.iou_target.ndim == 0 else "array%r" % (self.iou_target.shape,)
        return "Perturb(iou_target=%s, seed=%d, rounds=%d, min_size=%d, max_size=%d%s)" % (
            t, self.seed, self.rounds, self.min_size, self.max_size, "" if self.seeds is None else ", seeds=array%r" % (self.seeds.shape,))
