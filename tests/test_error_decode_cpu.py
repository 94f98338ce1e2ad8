"""CPU: the predicted error maps (INTEGRATION.md "Predicted error maps"; csrc/errhead.hip) - the numpy statements of the four
kernels that tests/test_gpu_error_decode.py compares the HIP kernels against, the host module quber_amd/eval/error_maps.py, the
four ABI entries and the public switches."""
import ctypes
import inspect

import numpy as np
import torch

from oracle import errmaps_np
from quber_amd import _lib, synth
from quber_amd.eval import error_maps as em


# ---- numpy statements of the kernels ----
def decode_np(logits, first, classes):
    """logits f32 [B,P,H,W] -> (u8 [B,H,W], int64 [B,classes]): torch.argmax over planes first .. first + classes - 1 (first index
    wins ties, NaN is the maximum) and the pixels per class."""
    cls = torch.argmax(torch.from_numpy(np.ascontiguousarray(logits[:, first:first + classes])), dim=1).numpy().astype(np.uint8)
    hist = np.stack([np.bincount(c.ravel(), minlength=classes) for c in cls])
    return cls, hist


def mask_hist_np(cls, masks, classes):
    """cls u8 [B,H,W], masks [B,N,H,W] (non-zero = inside) -> int64 [B,N,classes]: pixels of mask n that carry class c."""
    B, N = masks.shape[:2]
    out = np.zeros((B, N, classes), np.int64)
    for b in range(B):
        for n in range(N):
            inside = masks[b, n] != 0
            for c in range(classes):
                out[b, n, c] = np.count_nonzero(inside & (cls[b] == c))
    return out


def confusion_np(cls, explicit, kind, error_type):
    """cls u8 [B,H,W], explicit u8 [B,2,4,H,W] -> int64 [B,C+1,C]: row = target class (em.target_class_map; row C = none),
    column = predicted class; a predicted class >= C is counted nowhere."""
    C = em.n_classes(error_type)
    tgt = em.target_class_map(explicit[:, kind], error_type)
    out = np.zeros((cls.shape[0], C + 1, C), np.int64)
    for b in range(cls.shape[0]):
        for t in range(C + 1):
            for p in range(C):
                out[b, t, p] = np.count_nonzero((tgt[b] == t) & (cls[b] == p))
    return out


def overlay_np(bgr, cls, palette):
    """bgr u8 [B,H,W,3], cls u8 [B,H,W], palette: per class a (B, G, R) colour or None -> u8 [B,H,W,3]."""
    out = np.array(bgr, dtype=np.uint8)
    for c, col in enumerate(palette):
        if col is not None:
            out[cls == c] = col
    return out


# ---- the statements themselves ----
def test_decode_np_ties_and_nans():
    nan, inf = np.nan, np.inf
    px = np.array([[0.0, -0.0, 0.0, 0.0],      # all tie: first
                   [1.0, 2.0, 2.0, 1.0],       # first of the two maxima
                   [1.0, nan, inf, nan],       # the first NaN beats +inf
                   [-inf, -inf, -inf, -inf],
                   [-0.0, 0.0, -1.0, 0.0]], np.float32)
    lg = np.zeros((1, 6, 1, 5), np.float32)
    lg[0, 2:6, 0, :] = px.T
    cls, hist = decode_np(lg, 2, 4)
    assert cls[0, 0].tolist() == [0, 1, 1, 0, 0] and hist.tolist() == [[3, 2, 0, 0]]
    cls3, hist3 = decode_np(lg, 3, 3)
    assert cls3[0, 0].tolist() == [0, 0, 0, 0, 0] and hist3.tolist() == [[5, 0, 0]]


def test_target_class_map_is_the_reference_training_target():
    """model.py:185-227 builds the target stack per error type by concatenating (sums of) the TP / TN / FP / FN planes; the class a
    pixel trains towards is the index of its set plane in that stack."""
    sc = synth.make_scene(4, 96, 128, 5)
    gt = synth.make_scene(9, 96, 128, 4)["masks"]
    ex = errmaps_np.explicit_error_maps((sc["masks"] != 0).astype(np.uint8), (gt != 0).astype(np.uint8))
    for kind in (0, 1):
        tp, tn, fp, fn = (ex[kind, i] for i in range(4))
        assert np.array_equal(tp + tn + fp + fn, np.ones_like(tp))           # one-hot
        stacks = {"e3": [tp, tn, fp, fn], "e2": [tp + tn, fp + fn], "e33": [tp + tn, fp, fn], "e32": [fp, fn]}
        for et in em.ERROR_TYPES:
            st = np.stack(stacks[et])
            assert st.shape[0] == em.n_classes(et) == len(em.CLASS_NAMES[et])
            got = em.target_class_map(ex[kind], et)
            none = st.sum(0) == 0
            assert np.array_equal(got[none], np.full(int(none.sum()), st.shape[0], np.uint8))
            assert np.array_equal(got[~none], st.argmax(0)[~none]) and np.all(st.sum(0) <= 1)
            assert bool(none.any()) == (et == "e32")
            if et == "e32":
                assert np.array_equal(none, (tp + tn) == 1) and none.sum() > 0
        # each class is populated on this scene: the check above is not vacuous
        assert all(int(ex[kind, i].sum()) > 0 for i in range(4))
    # batched input, and a pixel with no plane set
    exb = np.stack([ex, ex])
    assert np.array_equal(em.target_class_map(exb[:, 1], "e33")[1], em.target_class_map(ex[1], "e33"))
    assert em.target_class_map(np.zeros((4, 2, 2), np.uint8), "e3").tolist() == [[4, 4], [4, 4]]
    assert em.target_class_map(np.full((4, 1, 1), 255, np.uint8), "e3").tolist() == [[0]]


def test_iou_from_confusion_hand_tables():
    # e3: rows TP, TN, FP, FN (+ none), columns predicted
    t = np.array([[5, 0, 1, 0],
                  [0, 80, 0, 0],
                  [2, 0, 6, 0],
                  [0, 3, 0, 0],       # FN never predicted right
                  [0, 0, 0, 0]])
    r = em.iou_from_confusion(t)
    np.testing.assert_allclose(r["iou"], [5 / 8, 80 / 83, 6 / 9, 0.0])
    np.testing.assert_allclose(r["iou_all"], 91 / (8 + 83 + 9 + 3))
    np.testing.assert_allclose(r["accuracy"], 91 / 97)
    np.testing.assert_allclose(em.iou_err(t, "e3"), 6 / (9 + 3))
    # e32 with the extra row populated: it changes nothing; class 1 has an empty union -> NaN
    t32 = np.array([[4, 0], [0, 0], [7, 9]])
    r = em.iou_from_confusion(t32)
    assert r["iou"][0] == 1.0 and np.isnan(r["iou"][1]) and r["iou_all"] == 1.0 and r["accuracy"] == 1.0
    assert em.iou_err(t32, "e32") == 1.0
    same = em.iou_from_confusion(np.array([[4, 0], [0, 0], [0, 0]]))
    assert same["iou_all"] == r["iou_all"] and same["accuracy"] == r["accuracy"]
    # nothing at all
    z = em.iou_from_confusion(np.zeros((3, 2), np.int64))
    assert np.isnan(z["iou"]).all() and np.isnan(z["iou_all"]) and np.isnan(z["accuracy"]) and np.isnan(em.iou_err(np.zeros((3, 2)), "e2"))
    # e2: error class = index 1; batched tables
    t2 = np.array([[[10, 2], [1, 3], [0, 0]], [[0, 0], [0, 5], [0, 0]]])
    np.testing.assert_allclose(em.iou_err(t2, "e2"), [3 / 6, 1.0])
    np.testing.assert_allclose(em.iou_from_confusion(t2)["iou_all"], [13 / (13 + 3 + 3), 1.0])
    assert em.error_class_indices("e3") == [2, 3] and em.error_class_indices("e33") == [1, 2] and em.error_class_indices("e32") == [0, 1]


def test_mask_error_ratio_hand_rows():
    h = np.array([[30, 5, 10, 2], [0, 0, 0, 0], [0, 7, 0, 9], [0, 0, 4, 0]])          # e3: TP, TN, FP, FN
    r = em.mask_error_ratio(h, "e3")
    np.testing.assert_allclose(r[[0, 3]], [10 / 40, 1.0])
    assert np.isnan(r[1]) and np.isnan(r[2])                  # an empty mask; a mask with no TP / FP pixel
    np.testing.assert_allclose(em.mask_error_ratio(np.array([[6, 2], [0, 0]]), "e2"), [0.25, np.nan])
    np.testing.assert_allclose(em.mask_error_ratio(np.array([[6, 2, 50]]), "e33"), [0.25])
    np.testing.assert_allclose(em.mask_error_ratio(np.array([[[3, 1]]]), "e32"), [[0.75]])


def test_default_palette_is_the_reference_picture():
    assert em.ERROR_TYPES == ("e3", "e2", "e33", "e32")
    assert em.DEFAULT_PALETTE["e3"] == ((0, 255, 0), None, (0, 0, 255), (255, 0, 0))       # eval/eval_utils.py:315-317
    for et in em.ERROR_TYPES:
        assert len(em.DEFAULT_PALETTE[et]) == em.n_classes(et)
        for i, col in enumerate(em.DEFAULT_PALETTE[et]):
            assert (col is not None) == (i in em.error_class_indices(et)) or (et == "e3" and i == 0)
    bgr = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(1, 2, 3, 3)
    cls = np.array([[[0, 1, 2], [3, 1, 7]]], np.uint8)
    out = overlay_np(bgr, cls, em.DEFAULT_PALETTE["e3"])
    assert out[0, 0].tolist() == [[0, 255, 0], [3, 4, 5], [0, 0, 255]] and out[0, 1].tolist() == [[255, 0, 0], [12, 13, 14], [15, 16, 17]]


# ---- ABI and public switches ----
ENTRIES = ("quber_error_decode", "quber_error_mask_hist", "quber_error_score", "quber_error_overlay")


def test_signatures_and_library_exports():
    P, I, U = _lib._P, _lib._I, ctypes.c_uint32
    assert _lib.SIGNATURES["quber_error_decode"] == (ctypes.c_int, [P, P, I, I, I, I, P, P, P])
    assert _lib.SIGNATURES["quber_error_mask_hist"] == (ctypes.c_int, [P, P, P, I, I, I, P, P])
    assert _lib.SIGNATURES["quber_error_score"] == (ctypes.c_int, [P, P, P, I, I, I, I, P, P])
    assert _lib.SIGNATURES["quber_error_overlay"] == (ctypes.c_int, [P, P, P, I, U, U, U, U, P, P])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name


def test_null_context_fails_loudly():
    lib = _lib.load()
    assert lib.quber_error_decode(None, None, 8, 4, 4, 1, None, None, None) != 0
    assert b"null context" in lib.quber_last_error()
    assert lib.quber_error_mask_hist(None, None, None, 1, 1, 4, None, None) != 0
    assert lib.quber_error_score(None, None, None, 1, 0, 4, 1, None, None) != 0
    assert lib.quber_error_overlay(None, None, None, 1, 0, 0, 0, 0, None, None) != 0


def test_decode_errors_keyword_defaults_off():
    from quber_amd.eval.refiner_model import MaskRefiner, MaskRefinerTTA
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor, RefinerModel
    for cls in (MaskRefinerPredictor, RefinerModel, MaskRefiner, MaskRefinerTTA):
        p = inspect.signature(cls.__init__).parameters
        assert "decode_errors" in p and p["decode_errors"].default is False, cls
    assert RefinerModel(None, {}, "cpu").decode_errors is False
    assert RefinerModel(None, {}, "cpu", decode_errors=True).decode_errors is True
    assert RefinerModel(None, {}, "cpu").decode(None, None) is None          # off: nothing is enqueued
    for name in ("score_error_maps", "visualize_errors"):
        assert callable(getattr(MaskRefiner, name))
