"""Scene-level perturbation of a frame's instance list (csrc/scene.hip; INTEGRATION.md "Scene-level perturbation"): the part of the
reference's tools/ours/perturbate_masks.py:101-205 that works on the list - false positives and over- / under-segmentations from a pool
of proposals, merging of close masks, splits along an axis-aligned line, deletions - split into the part that draws random numbers -
here, on the host - and the part that touches pixels - ``Engine.scene_perturb``, on the device.  Plain host-side data, like
``perturb.Perturb``.

The reference draws from Python's ``random`` and how many numbers it consumes depends on the data (a coin per proposal that is then
filtered or not, up to ten attempts per split), so its stream cannot be reproduced and is not.  Every decision it takes is an
independent draw, though: a table with one draw per (stage, slot, attempt) has the same distribution.  ``scene_draws`` is that table."""
import numbers

import numpy as np

MAX_SLOTS = 256            # csrc/scene.hip: SC_MAX - the bound of n_gt + n_prop and of max_masks
ATTEMPTS = 10              # perturbate_masks.py:168
RATIOS = ("fp", "gs", "merge", "split", "delete")
DEFAULT_RANGES = {"fp": (0.0, 0.2), "gs": (0.0, 0.3), "merge": (0.0, 0.1), "split": (0.0, 0.1), "delete": (0.0, 0.1)}   # :24-28
WALK_RANGE = (0.8, 1.0)    # :29 iou_target_range


def _ratio(name, v):
    """A number, or a (lo, hi) range, in 0 .. 1 -> float | (float, float)."""
    def num(x):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, numbers.Real) or not np.isfinite(x) or not 0.0 <= x <= 1.0:
            raise ValueError(f"scene: {name} must be a number in 0 .. 1 or a (lo, hi) range of such numbers")
        return float(x)
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"scene: {name} must be a number in 0 .. 1 or a (lo, hi) range of such numbers")
        lo, hi = num(v[0]), num(v[1])
        if lo > hi:
            raise ValueError(f"scene: {name}: lo > hi")
        return lo, hi
    return num(v)


def scene_draws(rng, n_prop, M, h, w, fp=DEFAULT_RANGES["fp"], gs=DEFAULT_RANGES["gs"], merge=DEFAULT_RANGES["merge"],
                split=DEFAULT_RANGES["split"], delete=DEFAULT_RANGES["delete"]):
    """Every random decision of one frame, drawn up front from ``rng`` (a ``numpy.random.RandomState``) in this order:

        1. the ratios fp, gs, merge, split, delete: ``rng.uniform(lo, hi)`` for a (lo, hi) range, NO draw for a plain number
        2. fp_act[n_prop]      = rng.random_sample(n_prop) <= fp ratio          5. split_act[M]  = rng.random_sample(M) <= split ratio
        3. gs_act[n_prop]      = rng.random_sample(n_prop) <= gs ratio          6. split_try[M][10][4], per slot, per attempt: x1 = rng.randint(w),
        4. merge_act[M]        = rng.random_sample(M) <= merge ratio               y1 = rng.randint(h), axis = 0 if rng.random_sample() < 0.5 else 1,
                                                                                   side = 0 if rng.random_sample() < 0.5 else 1
        7. delete_act[M]       = rng.random_sample(M) <= delete ratio           8. walk_targets[M] = rng.uniform(0.8, 1.0, M)

    ``act = draw <= ratio``: the reference skips on ``random.random() > ratio``.  axis 0 cuts rows, axis 1 columns; side 0 cuts from the
    line to the far edge, side 1 from the near edge to the line (perturbate_masks.py:178-187: the first coin picks the axis, the second
    the side; its unused x2, y2 are not drawn).  -> dict of ratios f64 [5], fp_act / gs_act u8 [n_prop], merge_act / split_act /
    delete_act u8 [M], split_try i32 [M,10,4] with the rows (x1, y1, axis, side), walk_targets f64 [M]."""
    ratios = np.empty((5,), np.float64)
    for i, r in enumerate((fp, gs, merge, split, delete)):
        r = _ratio(RATIOS[i], r)
        ratios[i] = rng.uniform(r[0], r[1]) if isinstance(r, tuple) else r
    fp_act = rng.random_sample(n_prop) <= ratios[0]
    gs_act = rng.random_sample(n_prop) <= ratios[1]
    merge_act = rng.random_sample(M) <= ratios[2]
    split_act = rng.random_sample(M) <= ratios[3]
    split_try = np.empty((M, ATTEMPTS, 4), np.int32)
    for k in range(M):
        for a in range(ATTEMPTS):
            x1 = rng.randint(w)
            y1 = rng.randint(h)
            axis = 0 if rng.random_sample() < 0.5 else 1
            side = 0 if rng.random_sample() < 0.5 else 1
            split_try[k, a] = (x1, y1, axis, side)
    delete_act = rng.random_sample(M) <= ratios[4]
    walk_targets = rng.uniform(WALK_RANGE[0], WALK_RANGE[1], M)
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    return {"ratios": ratios, "fp_act": u8(fp_act), "gs_act": u8(gs_act), "merge_act": u8(merge_act), "split_act": u8(split_act),
            "split_try": split_try, "delete_act": u8(delete_act), "walk_targets": np.ascontiguousarray(walk_targets, dtype=np.float64)}


class ScenePerturb:
    """seed: frame b of a call draws from ``RandomState(seed + b)`` (``scene_draws``).  max_masks: the capacity M of the perturbed list -
    the mask rows of a predictor pass; an append beyond it is not performed and counted in the report's ``dropped``.  min_mask_ratio: a
    proposal, and either half of a split, must cover that share of the frame (the reference's 0.01; a split compares 255 x pixels).
    fp / gs / merge / split / delete: the probability of each decision - a number, or the (lo, hi) range the frame's ratio is drawn
    from (defaults: the reference's ranges)."""

    __slots__ = ("seed", "max_masks", "min_mask_ratio", "ratios", "_cache", "_last")

    def __init__(self, seed=0, max_masks=64, min_mask_ratio=0.01, fp=DEFAULT_RANGES["fp"], gs=DEFAULT_RANGES["gs"],
                 merge=DEFAULT_RANGES["merge"], split=DEFAULT_RANGES["split"], delete=DEFAULT_RANGES["delete"]):
        def integer(name, v):                      # Python and numpy integers; no bool, no float
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral):
                raise ValueError(f"scene: {name} must be an integer")
            return int(v)
        seed, max_masks = integer("seed", seed), integer("max_masks", max_masks)
        if not 0 <= seed < 2 ** 31:
            raise ValueError("scene: seed must lie in 0 .. 2^31 - 1")
        if not 1 <= max_masks <= MAX_SLOTS:
            raise ValueError(f"scene: max_masks must lie in 1 .. {MAX_SLOTS}")
        r = min_mask_ratio
        if isinstance(r, (bool, np.bool_)) or not isinstance(r, numbers.Real) or not np.isfinite(r) or not 0.0 <= r <= 1.0:
            raise ValueError("scene: min_mask_ratio must be a number in 0 .. 1")
        self.seed, self.max_masks, self.min_mask_ratio = seed, max_masks, float(r)
        self.ratios = tuple(_ratio(n, v) for n, v in zip(RATIOS, (fp, gs, merge, split, delete)))
        self._cache = {}
        self._last = None

    @classmethod
    def parse(cls, value):
        """None | ScenePerturb -> None | ScenePerturb."""
        if value is None or isinstance(value, cls):
            return value
        raise ValueError(f"scene={value!r}: expected None or a quber_amd.scene.ScenePerturb")

    def draws(self, frames, n_prop, h, w):
        """The tables of a call of `frames` frames with n_prop proposal rows at h x w: scene_draws() of RandomState(seed + b), stacked ->
        dict of ratios f64 [frames,5], fp_act / gs_act u8 [frames,n_prop], merge_act / split_act / delete_act u8 [frames,M], split_try
        i32 [frames,M,10,4], walk_targets f64 [frames,M].  A pure function of the arguments and the options, so the result is kept."""
        key = (int(frames), int(n_prop), int(h), int(w))
        if key not in self._cache:
            if len(self._cache) >= 8:
                self._cache.pop(next(iter(self._cache)))
            if key[0] < 1:
                raise ValueError("scene: draws for less than one frame")
            per = [scene_draws(np.random.RandomState(self.seed + b), key[1], self.max_masks, key[2], key[3], *self.ratios) for b in range(key[0])]
            out = {k: np.ascontiguousarray(np.stack([p[k] for p in per])) for k in per[0]}
            for a in out.values():
                a.setflags(write=False)
            self._cache[key] = out
        self._last = key[1:]
        return self._cache[key]

    def walk_targets(self, frames, n_prop=None, h=None, w=None):
        """f64 [frames, M]: draw 8 of every frame - the IoU targets of perturbate_masks.py:208-210, so that
        ``Perturb(scene.walk_targets(B, P, H, W), ...)`` after this stage is the reference's last step.  The draws before them depend on
        the number of proposal rows and on the frame size (``randint`` consumes a bound-dependent share of the stream): n_prop, h and w
        default to those of the latest ``draws`` call, and are required before there has been one."""
        if n_prop is None or h is None or w is None:
            if self._last is None or not (n_prop is None and h is None and w is None):
                raise ValueError("scene: walk_targets needs n_prop, h and w (all three) before the first call has fixed them")
            n_prop, h, w = self._last
        return self.draws(frames, n_prop, h, w)["walk_targets"].copy()

    def _key(self):
        return (self.seed, self.max_masks, self.min_mask_ratio, self.ratios)

    def __eq__(self, other):
        return isinstance(other, ScenePerturb) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "ScenePerturb(seed=%d, max_masks=%d, min_mask_ratio=%r, %s)" % (
            self.seed, self.max_masks, self.min_mask_ratio, ", ".join("%s=%r" % (n, r) for n, r in zip(RATIOS, self.ratios)))
