"""CPU: horizontal-flip test-time augmentation (INTEGRATION.md "Test-time augmentation") - the two ABI entries, the public
constructors, and the numpy statement of the merge that tests/test_gpu_tta.py compares the HIP kernel against."""
import ctypes
import inspect
import os
import re

import numpy as np

from conftest import ROOT
from quber_amd import _lib

X_OFFSET_PLANE = 3      # plane order fg, centre, off_y, off_x (csrc/postproc.hip)


def tta_merge_np(logits2):
    """The contract: logits2 f32 [2B,P,H,W] (originals in [0,B), their W-mirrors in [B,2B)) -> f32 [B,P,H,W],
    out[b,c,y,x] = (L[b,c,y,x] + s_c * L[B+b,c,y,W-1-x]) * 0.5f, s_c = -1 on the x-offset plane, +1 on every other one."""
    L = np.asarray(logits2, dtype=np.float32)
    B = L.shape[0] // 2
    s = np.ones(L.shape[1], np.float32)
    s[X_OFFSET_PLANE] = -1.0
    out = (L[:B] + s[None, :, None, None] * L[B:, :, :, ::-1]) * np.float32(0.5)
    assert out.dtype == np.float32
    return out


def mirror_logits_np(logits):
    """What the W-mirror of a frame does to its logits: every plane mirrored along W, the x-offset plane negated."""
    L = np.array(np.asarray(logits, np.float32)[..., ::-1])
    L[:, X_OFFSET_PLANE] = -L[:, X_OFFSET_PLANE]
    return L


def _header():
    return open(os.path.join(ROOT, "include", "quber_hip.h")).read()


def test_header_declares_the_tta_entries_and_cites_the_reference():
    txt = _header()
    assert re.search(r"int quber_tta_flip_inputs\(quber_ctx\* ctx, uint8_t\* dev_bgr, uint8_t\* dev_depth, uint8_t\* dev_masks, "
                     r"int32_t batch,\s+int32_t n_masks, void\* stream\);", txt)
    assert re.search(r"int quber_tta_merge\(quber_ctx\* ctx, const float\* dev_logits2, int32_t n_planes, int32_t batch, "
                     r"float\* dev_out,\s+void\* stream\);", txt)
    for cite in ("eval/un_eval_utils.py:78-81", "maskrefiner/test_time_augmentation.py:72-95", "model.py:304-307",
                 "maskrefiner/predictor.py:304-348"):
        assert cite in txt, cite


def test_signatures_and_library_exports():
    assert _lib.SIGNATURES["quber_tta_flip_inputs"] == (ctypes.c_int, [_lib._P] * 4 + [_lib._I, _lib._I, _lib._P])
    assert _lib.SIGNATURES["quber_tta_merge"] == (ctypes.c_int, [_lib._P, _lib._P, _lib._I, _lib._I, _lib._P, _lib._P])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "quber_tta_flip_inputs") and hasattr(lib, "quber_tta_merge")
    loaded = _lib.load()
    assert loaded.quber_tta_merge.argtypes == _lib.SIGNATURES["quber_tta_merge"][1]


def test_null_context_fails_loudly():
    lib = _lib.load()
    assert lib.quber_tta_flip_inputs(None, None, None, None, 1, 0, None) != 0
    assert b"null context" in lib.quber_last_error()
    assert lib.quber_tta_merge(None, None, 8, 1, None, None) != 0


def test_mask_refiner_tta_is_the_reference_drivers_refiner():
    from quber_amd.eval.refiner_model import MaskRefiner, MaskRefinerTTA
    assert issubclass(MaskRefinerTTA, MaskRefiner)
    sig = inspect.signature(MaskRefinerTTA.__init__)
    # eval/un_eval_utils.py:79-81: MaskRefinerTTA(args.config_file, weights_file=args.weights_file, dataset=args.test_dataset)
    sig.bind(None, "configs/x.yaml", weights_file="model_final.pth", dataset="OCID")
    assert sig.parameters["weights_file"].default is None and sig.parameters["dataset"].default == "OSD"
    for name in ("predict", "predict_stream"):
        assert getattr(MaskRefinerTTA, name) is getattr(MaskRefiner, name)


def test_tta_keyword_defaults_off():
    from quber_amd.eval.refiner_model import MaskRefiner
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor, RefinerModel
    for cls in (MaskRefinerPredictor, MaskRefiner, RefinerModel):
        p = inspect.signature(cls.__init__).parameters
        assert "tta" in p and p["tta"].default is False, cls
    assert RefinerModel(None, {}, "cpu").tta is False
    assert RefinerModel(None, {}, "cpu", tta=True).tta is True


def test_merge_formula_np():
    rng = np.random.default_rng(0)
    B, P, H, W = 2, 8, 3, 5
    x = rng.normal(0, 3, (B, P, H, W)).astype(np.float32)
    # a frame whose mirrored pass returns exactly the mirrored logits merges into itself, bit for bit
    got = tta_merge_np(np.concatenate([x, mirror_logits_np(x)]))
    np.testing.assert_array_equal(got.view(np.uint32), x.view(np.uint32))
    # one element by hand, in float32: the add rounds once, the halving is exact
    L2 = rng.normal(0, 3, (2 * B, P, H, W)).astype(np.float32)
    out = tta_merge_np(L2)
    for b, c, y, xx in ((0, 0, 1, 0), (1, 3, 2, 4), (1, 7, 0, 2)):
        s = np.float32(-1.0 if c == X_OFFSET_PLANE else 1.0)
        exp = np.float32(np.float32(L2[b, c, y, xx] + s * L2[B + b, c, y, W - 1 - xx]) * np.float32(0.5))
        assert out[b, c, y, xx].view(np.uint32) == exp.view(np.uint32)
    # the merge of x with a mirrored pass commutes with the mirror (the flip-equivariance the GPU test measures)
    f = rng.normal(0, 3, (B, P, H, W)).astype(np.float32)
    a = tta_merge_np(np.concatenate([x, f]))
    b = tta_merge_np(np.concatenate([f, x]))
    np.testing.assert_array_equal(mirror_logits_np(b).view(np.uint32), a.view(np.uint32))
