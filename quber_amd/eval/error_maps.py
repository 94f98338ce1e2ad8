"""Host side of the predicted error maps (numpy only; importable without a GPU): class names and palettes per ERROR_TYPE, the
host statement of the target-class mapping ``quber_error_score`` applies on the device, and the metrics derived from its confusion
table and from the per-mask class histogram of ``quber_error_mask_hist``.

The two figures the reference reports per error head (explicit_error_estimation/util.py:38-42: ``iou_all`` over all classes,
``iou`` with the first class ignored) come from ``segmentation_models_pytorch``, which is not available here; they are defined
from the confusion table instead: micro IoU = sum_c tp_c / sum_c (tp_c + fp_c + fn_c) over the chosen classes.
"""
import numpy as np

# INS_EMBED_HEAD.ERROR_TYPE, in the order of the `error_type` argument of quber_error_score
ERROR_TYPES = ("e3", "e2", "e33", "e32")

# class names in plane order: the training-target stacks of maskrefiner/modeling/mask_refiner/model.py:185-227
CLASS_NAMES = {
    "e3": ("TP", "TN", "FP", "FN"),
    "e2": ("correct", "error"),
    "e33": ("correct", "FP", "FN"),
    "e32": ("FP", "FN"),
}

_CORRECT = ("TP", "TN", "correct")

# BGR colour per class, None = not painted.  e3: eval/eval_utils.py:315-317 (TP green, FP red, FN blue, TN untouched); the other
# error types paint their error classes only.
DEFAULT_PALETTE = {
    "e3": ((0, 255, 0), None, (0, 0, 255), (255, 0, 0)),
    "e2": (None, (0, 255, 255)),
    "e33": (None, (0, 0, 255), (255, 0, 0)),
    "e32": ((0, 0, 255), (255, 0, 0)),
}


def n_classes(error_type):
    return len(CLASS_NAMES[error_type])


def target_class_map(explicit_onehot, error_type):
    """explicit_onehot: [..., 4, H, W] planes (TP, TN, FP, FN), non-zero = set -> uint8 [..., H, W]: the index of the first set plane
    of the error type's target stack (model.py:185-227), ``n_classes(error_type)`` where the stack is all zero (e32 on TP / TN
    pixels; any type on a pixel with no plane set)."""
    e = np.asarray(explicit_onehot) != 0
    tp, tn, fp, fn = (e[..., i, :, :] for i in range(4))
    stack = {"e3": (tp, tn, fp, fn), "e2": (tp | tn, fp | fn), "e33": (tp | tn, fp, fn), "e32": (fp, fn)}[error_type]
    out = np.full(tp.shape, len(stack), np.uint8)
    for i in reversed(range(len(stack))):
        out[stack[i]] = i
    return out


def error_class_indices(error_type):
    """The classes that are errors: every class except TP / TN / "correct"."""
    return [i for i, n in enumerate(CLASS_NAMES[error_type]) if n not in _CORRECT]


def iou_from_confusion(table):
    """table: [..., C+1, C] confusion counts (row = target class, row C = pixels without a target - excluded from every figure -,
    column = predicted class) -> dict: ``iou`` per class [..., C] (tp / (tp + fp + fn), NaN where the union is empty), ``iou_all``
    micro IoU over all classes, ``accuracy``.  ``iou_err(table, error_type)`` is the micro IoU over the error classes."""
    t = np.asarray(table, dtype=np.float64)
    C = t.shape[-1]
    m = t[..., :C, :]
    tp = np.diagonal(m, axis1=-2, axis2=-1)
    fp = m.sum(-2) - tp            # predicted c, target another class
    fn = m.sum(-1) - tp            # target c, predicted another class
    union = tp + fp + fn
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.where(union > 0, tp / union, np.nan)
        iou_all = np.where(union.sum(-1) > 0, tp.sum(-1) / union.sum(-1), np.nan)
        total = m.sum((-2, -1))
        acc = np.where(total > 0, tp.sum(-1) / total, np.nan)
    return {"iou": iou, "iou_all": iou_all, "accuracy": acc}


def iou_err(table, error_type):
    """Micro IoU over the error classes only (util.py:40-41 ignores the first class; here: every class that is not TP / TN /
    "correct"); NaN when their union is empty."""
    t = np.asarray(table, dtype=np.float64)
    C = t.shape[-1]
    m = t[..., :C, :]
    idx = error_class_indices(error_type)
    tp = np.diagonal(m, axis1=-2, axis2=-1)[..., idx]
    union = (m.sum(-2) + m.sum(-1))[..., idx] - tp
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(union.sum(-1) > 0, tp.sum(-1) / union.sum(-1), np.nan)


def mask_error_ratio(mask_hist, error_type):
    """mask_hist: [..., N, C] pixels of initial mask n per predicted class -> [..., N]: rejected / (accepted + rejected), the share
    of the mask's pixels the network rejects.  A pixel inside an initial mask is TP or FP by construction, so the network rejects it
    with FP and accepts it with TP: e3 FP / (TP + FP), e33 FP / (correct + FP), e2 error / (correct + error); e32 has no accepting
    class, its ratio is FP / (FP + FN).  NaN for a mask without such pixels (an empty mask)."""
    h = np.asarray(mask_hist, dtype=np.float64)
    names = CLASS_NAMES[error_type]
    rej = names.index("error") if error_type == "e2" else names.index("FP")
    acc = {"e3": "TP", "e2": "correct", "e33": "correct", "e32": "FN"}[error_type]
    den = h[..., names.index(acc)] + h[..., rej]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, h[..., rej] / den, np.nan)
