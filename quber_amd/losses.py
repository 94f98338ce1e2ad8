"""Options of the validation losses (csrc/losses.hip; INTEGRATION.md "Validation losses"): the reference's training targets
(``PanopticDeepLabTargetGenerator``, maskrefiner/data/dataset_mappers/target_generator.py:8-165) and the five values of its loss dict
(maskrefiner/modeling/mask_refiner/model.py:36-72, 672-687, 766-802), per frame, on the device.  Plain host-side data, like
``masknms.MaskNMS``: the work is done by ``Engine.loss_targets`` and ``Engine.losses``."""
import ctypes as C
import functools
import numbers
from dataclasses import dataclass

import numpy as np

ERROR_TYPES = ("e3", "e2", "e33", "e32")                 # the C ABI's error_type = 0 .. 3
ERROR_CLASSES = {"e3": 4, "e2": 2, "e33": 3, "e32": 2}
LOSS_TYPES = ("dice", "cross_entropy")                   # the C ABI's loss type = 0, 1
LOSS_KEYS = ("loss_sem_seg", "loss_center", "loss_offset", "loss_eee_mask", "loss_eee_boundary")
HEADS = ("eee_mask", "eee_boundary")                     # region, boundary: plane 0 / 1 of the explicit error maps
MAX_SIGMA = 20                                           # csrc/losses.hip: the Gaussian table (6 sigma + 3)^2 floats sits in LDS
MAX_IDS = 254
TARGET_PLANES = ("center", "offset_y", "offset_x", "sem_seg", "sem_seg_weights", "inst_weights")
# the record of one frame: include/quber_hip.h QUBER_LOSS_WORDS float64 words
LOSS_WORDS = 40
W_FG_SUM, W_K, W_KTH, W_ABOVE, W_CENTER_NUM, W_WEIGHT_SUM, W_OFFSET_NUM, W_PIXELS = 5, 6, 7, 8, 9, 10, 11, 12
W_HEAD = {"eee_mask": 13, "eee_boundary": 26}            # ce_sum, inter[4], target_sum[4], prob_sum[4]


class LossSpec(C.Structure):
    """include/quber_hip.h: quber_loss_spec."""
    _fields_ = [("top_k", C.c_double), ("foreground_weight", C.c_double), ("center_weight", C.c_double), ("offset_weight", C.c_double),
                ("error_type", C.c_int32), ("eee_mask_plane", C.c_int32), ("eee_boundary_plane", C.c_int32), ("eee_mask_loss", C.c_int32),
                ("eee_boundary_loss", C.c_int32), ("reserved", C.c_int32)]


def _number(v, what, lo, hi, integer=False):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real) or (integer and int(v) != v):
        raise ValueError(f"losses: {what} must be {'an integer' if integer else 'a number'}")
    if not (np.isfinite(v) and lo <= v <= hi):
        raise ValueError(f"losses: {what}={v!r} outside {lo} .. {hi}")
    return int(v) if integer else float(v)


@functools.lru_cache(maxsize=None)
def gauss_table(sigma):
    """target_generator.py:46-51, rounded to float32 (the maximum of rounded values is the rounded maximum): f32 [(6 sigma + 3)^2]."""
    size, c = 6 * sigma + 3, 3 * sigma + 1
    x = np.arange(size, dtype=np.float64)
    g = np.exp(-((x - c) ** 2 + (x[:, None] - c) ** 2) / (2 * sigma ** 2)).astype(np.float32)
    g.setflags(write=False)
    return g


@dataclass(frozen=True)
class Losses:
    """sigma, small_area, small_weight: INPUT.GAUSSIAN_SIGMA / SMALL_INSTANCE_AREA / SMALL_INSTANCE_WEIGHT of the target generator.
    top_k, foreground_weight, center_weight, offset_weight: INS_EMBED_HEAD.FOREGROUND_LOSS_TOP_K and the three *_LOSS_WEIGHT.  The two eee
    loss types ("dice" | "cross_entropy") and weights: the weights are REPORTED beside the values, never applied - the reference does not
    apply them either (model.py:681, 686).  error_type: INS_EMBED_HEAD.ERROR_TYPE.  keep_targets: the predictor also returns the target
    planes of every frame."""
    sigma: int = 10
    small_area: int = 4096
    small_weight: float = 3
    top_k: float = 1.0
    foreground_weight: float = 1.0
    center_weight: float = 200.0
    offset_weight: float = 0.01
    eee_mask_loss_type: str = "dice"
    eee_mask_loss_weight: float = 1.0
    eee_boundary_loss_type: str = "dice"
    eee_boundary_loss_weight: float = 1.0
    error_type: str = "e3"
    foreground_loss_type: str = "hard_pixel_mining"
    keep_targets: bool = False

    def __post_init__(self):
        s = object.__setattr__
        s(self, "sigma", _number(self.sigma, "sigma", 1, MAX_SIGMA, integer=True))
        s(self, "small_area", _number(self.small_area, "small_area", 0, 2 ** 31 - 1, integer=True))
        s(self, "small_weight", _number(self.small_weight, "small_weight", 0.0, 2.0 ** 24))
        s(self, "top_k", _number(self.top_k, "top_k", 0.0, 1.0))
        if self.top_k == 0.0:
            raise ValueError("losses: top_k must be positive")
        for f in ("foreground_weight", "center_weight", "offset_weight", "eee_mask_loss_weight", "eee_boundary_loss_weight"):
            s(self, f, _number(getattr(self, f), f, -1e300, 1e300))
        for f in ("eee_mask_loss_type", "eee_boundary_loss_type"):
            if getattr(self, f) not in LOSS_TYPES:
                raise ValueError(f"losses: {f}={getattr(self, f)!r}: expected 'dice' or 'cross_entropy'")
        if self.error_type not in ERROR_TYPES:
            raise ValueError(f"losses: error_type={self.error_type!r}: expected one of {ERROR_TYPES}")
        if self.foreground_loss_type != "hard_pixel_mining":
            raise ValueError("losses: foreground_loss_type must be 'hard_pixel_mining' (the reference's one-plane foreground head cannot "
                             "run 'cross_entropy' either)")
        s(self, "keep_targets", bool(self.keep_targets))

    @classmethod
    def parse(cls, value):
        """None | Losses -> None | Losses."""
        if value is None or isinstance(value, cls):
            return value
        raise ValueError(f"losses={value!r}: expected None or a quber_amd.losses.Losses")

    @classmethod
    def from_cfg(cls, cfg, **over):
        """The reference's keys where the yaml has them, the defaults of its config.py otherwise; keywords override."""
        kw = {}
        if cfg is not None:
            inp, head = cfg.get("INPUT", {}), cfg.get("MODEL", {}).get("INS_EMBED_HEAD", {})
            for name, node, key in (("sigma", inp, "GAUSSIAN_SIGMA"), ("small_area", inp, "SMALL_INSTANCE_AREA"),
                                    ("small_weight", inp, "SMALL_INSTANCE_WEIGHT"), ("top_k", head, "FOREGROUND_LOSS_TOP_K"),
                                    ("foreground_weight", head, "FOREGROUND_LOSS_WEIGHT"), ("foreground_loss_type", head, "FOREGROUND_LOSS_TYPE"),
                                    ("center_weight", head, "CENTER_LOSS_WEIGHT"), ("offset_weight", head, "OFFSET_LOSS_WEIGHT"),
                                    ("eee_mask_loss_type", head, "EEE_MASK_LOSS_TYPE"), ("eee_mask_loss_weight", head, "EEE_MASK_LOSS_WEIGHT"),
                                    ("eee_boundary_loss_type", head, "EEE_BOUNDARY_LOSS_TYPE"),
                                    ("eee_boundary_loss_weight", head, "EEE_BOUNDARY_LOSS_WEIGHT"), ("error_type", head, "ERROR_TYPE")):
                if key in node:
                    kw[name] = node[key]
        kw.update(over)
        return cls(**kw)

    def top_k_pixels(self, numel):
        """model.py:70; 0 is refused (the reference would return the mean of nothing)."""
        k = numel if self.top_k == 1.0 else int(self.top_k * numel)
        if k < 1:
            raise ValueError(f"losses: top_k={self.top_k} selects no pixel of a frame of {numel}")
        return k

    def c_spec(self, heads):
        """heads: {"eee_mask" | "eee_boundary": first logit plane} -> the C ABI's quber_loss_spec."""
        return LossSpec(self.top_k, self.foreground_weight, self.center_weight, self.offset_weight, ERROR_TYPES.index(self.error_type),
                        int(heads.get("eee_mask", -1)), int(heads.get("eee_boundary", -1)), LOSS_TYPES.index(self.eee_mask_loss_type),
                        LOSS_TYPES.index(self.eee_boundary_loss_type), 0)

    def unpack(self, words, heads):
        """One frame's float64 record [LOSS_WORDS] (host) -> (losses {reference key: float}, loss_terms {...})."""
        w = [float(v) for v in words]
        out = {"loss_sem_seg": w[0], "loss_center": w[1], "loss_offset": w[2]}
        terms = {"fg_sum": w[W_FG_SUM], "k": int(w[W_K]), "kth": w[W_KTH], "above": int(w[W_ABOVE]), "center_num": w[W_CENTER_NUM],
                 "weight_sum": w[W_WEIGHT_SUM], "offset_num": w[W_OFFSET_NUM], "pixels": int(w[W_PIXELS])}
        ncls = ERROR_CLASSES[self.error_type]
        for i, head in enumerate(HEADS):
            if head in heads:
                o = W_HEAD[head]
                out["loss_" + head] = w[3 + i]
                terms[head] = {"ce_sum": w[o], "inter": w[o + 1:o + 1 + ncls], "target_sum": w[o + 5:o + 5 + ncls],
                               "prob_sum": w[o + 9:o + 9 + ncls], "loss_weight": getattr(self, head + "_loss_weight")}
        return out, terms
