"""Thin host-side driver of libquber_hip.so: owns one ``quber_ctx`` and hands torch (ROCm) tensors'
device pointers and the current HIP stream to the C ABI.  torch is plumbing only (device memory,
streams); every computation on the hot path happens in the HIP library.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from . import arch
from .cleanup import Cleanup
from .config import arch_kwargs


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def set_arch(qc, depth=50, backbone_fusion_layers=2, head_fusion_layers=3, error_classes=4, eee_mask_on=False,
             eee_boundary_on=True, hierarchical=True, hierarchy=arch.DEFAULT_HIERARCHY, fusion_target=("feat", "pred"),
             streams=2, fusion_add=False, convs_dim=128, head_channels=32):
    """Write the architecture switches (keyword arguments of arch.param_specs) into a quber_config."""
    qc.resnet_depth, qc.backbone_fusion_layers, qc.head_fusion_layers = depth, backbone_fusion_layers, head_fusion_layers
    qc.error_classes, qc.eee_mask_on, qc.eee_boundary_on = error_classes, int(eee_mask_on), int(eee_boundary_on)
    qc.hierarchical = int(hierarchical)
    qc.streams = streams
    qc.fusion_add = int(fusion_add)
    qc.convs_dim, qc.head_channels = int(convs_dim), int(head_channels)
    qc.fusion_feat, qc.fusion_pred = int("feat" in fusion_target), int("pred" in fusion_target)
    levels = list(hierarchy) if hierarchical else []
    qc.n_levels = len(levels)
    for i in range(5):
        for j in range(5):
            qc.level_heads[i][j] = -1
    for i, lvl in enumerate(levels):
        for j, k in enumerate(lvl):
            qc.level_heads[i][j] = arch.HEADS.index(k)
    return qc


# predictor.py:345-346 subtracts a float32 index array from a float64 scalar.  numpy < 2 (the reference pins 1.23.1,
# INSTALL.md:14) keeps that in float32 (value-based casting); numpy >= 2 promotes to float64.  The drop-in reproduces what
# the reference computes UNDER THE NUMPY OF THE CALLING PROCESS - so that swapping the predictor in changes no bit of a1 in
# either environment; QUBER_ENCODE_LEGACY_F32=0/1 overrides.  (C default: 0, the mode the golden fixtures pin.)
ENCODE_LEGACY_F32 = int(os.environ.get("QUBER_ENCODE_LEGACY_F32", int(np.lib.NumpyVersion(np.__version__) < "2.0.0")))


def make_config(height=480, width=640, max_batch=1, max_instances=64, cfg=None, with_network=True):
    """quber_config from an (optional) validated yaml CfgNode."""
    lib = _lib.load()
    qc = _lib.QuberConfig()
    lib.quber_default_config(C.byref(qc))
    qc.encode_legacy_f32 = ENCODE_LEGACY_F32
    qc.height, qc.width, qc.max_batch, qc.max_instances = height, width, max_batch, max_instances
    qc.with_network = 1 if with_network else 0
    if cfg is not None:
        m = cfg.MODEL
        set_arch(qc, **arch_kwargs(cfg))
        qc.res5_dilation = m.RESNETS.RES5_DILATION
        qc.gaussian_sigma = cfg.INPUT.get("GAUSSIAN_SIGMA", 10)
        qc.nms_kernel = m.PANOPTIC_DEEPLAB.NMS_KERNEL
        qc.top_k = m.PANOPTIC_DEEPLAB.TOP_K_INSTANCE
        qc.stuff_area = m.PANOPTIC_DEEPLAB.STUFF_AREA
        qc.center_threshold = m.PANOPTIC_DEEPLAB.CENTER_THRESHOLD
        for i in range(min(6, len(m.PIXEL_MEAN))):
            qc.pixel_mean[i] = float(m.PIXEL_MEAN[i])
            qc.pixel_std[i] = float(m.PIXEL_STD[i])
    return qc


def normalize_depth(depth, min_val=250.0, max_val=1500.0):
    """depth: device tensor uint16 / int16-viewed-as-uint16 / float32 [..., H, W] -> (u8 [..., H, W, 3], zero mask u8 [..., H, W]).
    Device-side eval/preprocess_utils.py:12-28."""
    lib = _lib.load()
    assert depth.is_cuda and depth.is_contiguous()
    if depth.dtype == torch.float32:
        is_float = 1
    elif depth.dtype in (torch.uint16, torch.int16):
        is_float = 0
    else:
        raise TypeError("normalize_depth expects uint16 or float32 depth")
    out = torch.empty(tuple(depth.shape) + (3,), dtype=torch.uint8, device=depth.device)
    zero = torch.empty(tuple(depth.shape), dtype=torch.uint8, device=depth.device)
    _lib.check(lib.quber_normalize_depth(_ptr(depth), is_float, depth.numel(), float(min_val), float(max_val), _ptr(out),
                                         _ptr(zero), _stream()))
    return out, zero


def resize_u8(img, dh, dw, linear=True):
    """cv2.resize(img, (dw, dh), interpolation=INTER_LINEAR | INTER_NEAREST) on the device: img u8 [H,W] or [H,W,C] tensor."""
    lib = _lib.load()
    assert img.is_cuda and img.dtype == torch.uint8 and img.is_contiguous() and img.dim() in (2, 3)
    ch = 1 if img.dim() == 2 else img.shape[2]
    out = torch.empty((dh, dw) + (() if img.dim() == 2 else (ch,)), dtype=torch.uint8, device=img.device)
    _lib.check(lib.quber_resize_u8(_ptr(img), img.shape[0], img.shape[1], ch, _ptr(out), dh, dw, int(bool(linear)), _stream()))
    return out


_INPAINT_WS = {}
_INPAINT_WS_MAX = 32       # ~22 MB each at 640x480


def inpaint_depth(depth3, kernel_size=3):
    """inpaint_depth of eval/preprocess_utils.py:44-64 on the device (csrc/inpaint_dev.hip; bit-equal to the host restatement
    quber_inpaint_depth_u8): depth3 u8 [H,W,3] or [B,H,W,3] device tensor -> the same shape.  Asynchronous on the current stream."""
    lib = _lib.load()
    assert depth3.is_cuda and depth3.dtype == torch.uint8 and depth3.is_contiguous() and depth3.shape[-1] == 3 and depth3.dim() in (3, 4)
    B = 1 if depth3.dim() == 3 else depth3.shape[0]
    H, W = depth3.shape[-3], depth3.shape[-2]
    need = lib.quber_inpaint_depth_workspace_bytes(B, H, W)
    import threading
    # one workspace per (stream, calling thread): the launches of one call are ordered on their stream, but two threads that share
    # a stream interleave theirs
    key = (depth3.device, torch.cuda.current_stream().cuda_stream, threading.get_ident())
    ws = _INPAINT_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=depth3.device)
        _INPAINT_WS.pop(key, None)
        while len(_INPAINT_WS) >= _INPAINT_WS_MAX:          # worker threads and side streams come and go (predict_stream): oldest first
            _INPAINT_WS.pop(next(iter(_INPAINT_WS)))
        _INPAINT_WS[key] = ws
    out = torch.empty_like(depth3)
    _lib.check(lib.quber_inpaint_depth_device(_ptr(depth3), B, H, W, int(kernel_size), _ptr(ws), ws.numel(), _ptr(out), _stream()))
    return out


class Engine:
    """One context on the current device.  All methods are asynchronous on torch's current stream."""

    def __init__(self, qcfg, device=None):
        if not torch.cuda.is_available():
            raise _lib.QuberError("quber_amd needs a ROCm GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.qcfg = qcfg
        self.H, self.W = qcfg.height, qcfg.width
        self.planes = 4 + qcfg.error_classes * (int(bool(qcfg.eee_mask_on)) + int(bool(qcfg.eee_boundary_on)))
        self.cap = qcfg.top_k
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_create(C.byref(qcfg), C.byref(h)))
        self.h = h
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            torch.cuda.synchronize(self.device)
            self.lib.quber_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- options (include/quber_hip.h: the keys of quber_set_option) ----
    def set_option(self, key, value):
        """This engine only.  Plan-time keys must be set before load_state_dict(); launch-time keys any time."""
        _lib.check(self.lib.quber_set_option(self.h, int(key), int(value)))

    def get_option(self, key):
        v = C.c_int32()
        _lib.check(self.lib.quber_get_option(self.h, int(key), C.byref(v)))
        return v.value

    # ---- weights ----
    def weight_specs(self):
        out = []
        name, numel = C.c_char_p(), C.c_int64()
        for i in range(self.lib.quber_num_weights(self.h)):
            _lib.check(self.lib.quber_weight_spec(self.h, i, C.byref(name), C.byref(numel)))
            out.append((name.value.decode(), numel.value))
        return out

    def load_state_dict(self, sd):
        """sd: name -> numpy / torch array in torch layout (detectron2-compatible keys)."""
        for name, numel in self.weight_specs():
            if name not in sd:
                raise KeyError(f"state_dict lacks '{name}'")
            v = sd[name]
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            v = np.ascontiguousarray(v, dtype=np.float32)
            if v.size != numel:
                raise ValueError(f"'{name}' has {v.size} elements, expected {numel}")
            _lib.check(self.lib.quber_set_weight(self.h, name.encode(), C.c_void_p(v.ctypes.data), v.size))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_finalize_weights(self.h))

    def plan(self):
        """[(name, kind, flops at batch 1, launches)] of quber_forward in execution order."""
        out = []
        name, kind, fl, ln = C.c_char_p(), C.c_int32(), C.c_double(), C.c_int32()
        for i in range(self.lib.quber_num_ops(self.h)):
            _lib.check(self.lib.quber_op_info(self.h, i, C.byref(name), C.byref(kind), C.byref(fl), C.byref(ln)))
            out.append((name.value.decode(), ("conv", "norm", "other")[kind.value], fl.value, ln.value))
        return out

    def forward_flops(self):
        return self.lib.quber_forward_flops(self.h)

    def forward_flops_executed(self):
        return self.lib.quber_forward_flops_executed(self.h)

    def forward_flops_padding(self):
        """The part of forward_flops_executed() spent on the padding of Winograd tiles."""
        return self.lib.quber_forward_flops_padding(self.h)

    # ---- hot path ----
    def encode(self, masks, out=None):
        """masks u8 [B,N,H,W] (device) -> f32 [B,3,H,W]."""
        B, N = masks.shape[:2]
        assert masks.dtype == torch.uint8 and masks.is_contiguous() and masks.shape[2:] == (self.H, self.W)
        if out is None:
            out = torch.empty((B, 3, self.H, self.W), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.quber_encode_initial_masks(self.h, _ptr(masks), B, N, _ptr(out), _stream()))
        return out

    def encode_label_map(self, labels, n, out=None):
        """labels i32 [B,H,W] (device; 0 = none, 1..n = instance) -> f32 [B,3,H,W], as encode() on the masks (labels == i + 1)."""
        B = labels.shape[0]
        assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.shape[1:] == (self.H, self.W)
        if out is None:
            out = torch.empty((B, 3, self.H, self.W), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.quber_encode_label_map(self.h, _ptr(labels), B, n, _ptr(out), _stream()))
        return out

    def workspace_bytes(self):
        return self.lib.quber_workspace_bytes(self.h)

    def error_maps(self, init_masks, gt_masks, out=None):
        B, N = init_masks.shape[:2]
        Ng = gt_masks.shape[1]
        assert init_masks.dtype == torch.uint8 and gt_masks.dtype == torch.uint8
        assert init_masks.is_contiguous() and gt_masks.is_contiguous()
        if out is None:
            out = torch.empty((B, 2, 4, self.H, self.W), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.quber_explicit_error_maps(self.h, _ptr(init_masks), N, _ptr(gt_masks), Ng, B, _ptr(out),
                                                      _stream()))
        return out

    def forward(self, bgr, depth, offsets, out=None):
        """bgr, depth u8 [B,H,W,3] (depth None for a single-stream model: `bgr` is then THE image, rgb or depth);
        offsets f32 [B,3,H,W] -> logits f32 [B,planes,H,W]."""
        B = bgr.shape[0]
        assert bgr.dtype == torch.uint8 and offsets.dtype == torch.float32
        assert bgr.shape == (B, self.H, self.W, 3) and offsets.shape == (B, 3, self.H, self.W)
        assert bgr.is_contiguous() and offsets.is_contiguous()
        if self.qcfg.streams == 2:
            assert depth is not None and depth.dtype == torch.uint8 and depth.shape == bgr.shape and depth.is_contiguous()
        else:
            depth = None
        if out is None:
            out = torch.empty((B, self.planes, self.H, self.W), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.quber_forward(self.h, _ptr(bgr), _ptr(depth), _ptr(offsets), B, _ptr(out), _stream()))
        return out

    def forward_profiled(self, bgr, depth, offsets, out=None):
        """forward with HIP events around every launch group -> (logits, {kind: (ms, launches)})."""
        B = bgr.shape[0]
        if out is None:
            out = torch.empty((B, self.planes, self.H, self.W), dtype=torch.float32, device=self.device)
        ms, cnt = (C.c_double * 3)(), (C.c_int32 * 3)()
        _lib.check(self.lib.quber_forward_profiled(self.h, _ptr(bgr), _ptr(depth), _ptr(offsets), B, _ptr(out),
                                                   _stream(), C.byref(ms), C.byref(cnt)))
        return out, {k: (ms[i], cnt[i]) for i, k in enumerate(("conv", "norm", "other"))}

    def profile_begin(self):
        """Start a stage profile: every call on this engine until profile_end() brackets its kernels with HIP events."""
        _lib.check(self.lib.quber_profile_begin(self.h))

    def profile_end(self):
        """-> {stage: dict(ms, bytes, flops, launches)}; synchronises the current stream."""
        _lib.check(self.lib.quber_profile_end(self.h, _stream()))
        out = {}
        name, ms, by, fl, ln = C.c_char_p(), C.c_double(), C.c_double(), C.c_double(), C.c_int32()
        for i in range(self.lib.quber_profile_num_stages(self.h)):
            _lib.check(self.lib.quber_profile_stage(self.h, i, C.byref(name), C.byref(ms), C.byref(by), C.byref(fl), C.byref(ln)))
            out[name.value.decode()] = {"ms": ms.value, "bytes": by.value, "flops": fl.value, "launches": ln.value}
        return out

    def alloc_post(self, B):
        d, cap = self.device, self.cap
        return {
            "panoptic": torch.empty((B, self.H, self.W), dtype=torch.float32, device=d),
            "count": torch.empty((B,), dtype=torch.int32, device=d),
            "labels": torch.empty((B, cap), dtype=torch.float32, device=d),
            "scores": torch.empty((B, cap), dtype=torch.float32, device=d),
            "boxes": torch.empty((B, cap, 4), dtype=torch.float32, device=d),
            "centers": torch.zeros((B, cap, 2), dtype=torch.int32, device=d),
            "ncenters": torch.empty((B,), dtype=torch.int32, device=d),
        }

    def postprocess(self, logits, out=None):
        B, planes = logits.shape[:2]
        assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.shape[2:] == (self.H, self.W)
        o = out if out is not None else self.alloc_post(B)
        _lib.check(self.lib.quber_postprocess(
            self.h, _ptr(logits), planes, B, _ptr(o["panoptic"]), _ptr(o["count"]), _ptr(o["labels"]),
            _ptr(o["scores"]), _ptr(o["boxes"]), _ptr(o["centers"]), _ptr(o["ncenters"]), _stream()))
        return o

    # ---- horizontal-flip test-time augmentation: one forward of 2B frames, mirrors in slots [B, 2B) ----
    def tta_flip_inputs(self, bgr, depth, masks):
        """bgr (and depth, or None) u8 [2B,H,W,3], masks u8 [2B,N,H,W] or None (device): frames [0,B) are the caller's; their
        W-mirrors are written into [B,2B) in place.  encode() on all 2B frames afterwards gives the mirrored frames' a1."""
        B2 = bgr.shape[0]
        assert B2 % 2 == 0, "the test-time-augmentation buffers hold 2B frames"
        assert bgr.dtype == torch.uint8 and bgr.is_contiguous() and bgr.shape == (B2, self.H, self.W, 3)
        if depth is not None:
            assert depth.dtype == torch.uint8 and depth.is_contiguous() and depth.shape == bgr.shape
        n = 0
        if masks is not None:
            assert masks.dtype == torch.uint8 and masks.is_contiguous() and masks.shape[0] == B2 and masks.shape[2:] == (self.H, self.W)
            n = masks.shape[1]
        _lib.check(self.lib.quber_tta_flip_inputs(self.h, _ptr(bgr), _ptr(depth), _ptr(masks if n else None), B2 // 2, n,
                                                  _stream()))

    def tta_merge(self, logits, out=None):
        """logits f32 [2B,planes,H,W] of (originals, mirrors) -> f32 [B,planes,H,W]:
        (L[b] + s * mirror_W(L[B+b])) * 0.5, s = -1 on plane 3 (off_x), +1 elsewhere."""
        B2, planes = logits.shape[:2]
        assert B2 % 2 == 0, "the test-time-augmentation logits hold 2B frames"
        assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.shape[2:] == (self.H, self.W)
        if out is None:
            out = torch.empty((B2 // 2, planes, self.H, self.W), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (B2 // 2, planes, self.H, self.W)
        _lib.check(self.lib.quber_tta_merge(self.h, _ptr(logits), planes, B2 // 2, _ptr(out), _stream()))
        return out

    # ---- the predicted error maps on the device (csrc/errhead.hip; INTEGRATION.md "Predicted error maps") ----
    def error_heads(self):
        """{head name: (first logit plane, classes)} of the enabled error heads, in the plane order of QUBER_LOGIT_BASE:
        the boundary head first, then the region head."""
        qc, o, heads = self.qcfg, 4, {}
        if qc.eee_boundary_on:
            heads["eee_boundary"] = (o, qc.error_classes)
            o += qc.error_classes
        if qc.eee_mask_on:
            heads["eee_mask"] = (o, qc.error_classes)
        return heads

    def error_decode(self, logits, head, out=None, hist=None):
        """logits f32 [B,planes,H,W]; head: a name of error_heads() or (first_plane, classes) -> (class map u8 [B,H,W],
        pixels per class i32 [B,classes]); exactly torch.argmax(logits[:, first:first + classes], 1)."""
        first, ncls = self.error_heads()[head] if isinstance(head, str) else head
        B, planes = logits.shape[:2]
        assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.shape[2:] == (self.H, self.W)
        assert 2 <= ncls <= 4 and 0 <= first and first + ncls <= planes
        if out is None:
            out = torch.empty((B, self.H, self.W), dtype=torch.uint8, device=self.device)
        if hist is None:
            hist = torch.empty((B, ncls), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == (B, self.H, self.W)
        assert hist.dtype == torch.int32 and hist.is_contiguous() and hist.shape == (B, ncls)
        _lib.check(self.lib.quber_error_decode(self.h, _ptr(logits), planes, first, ncls, B, _ptr(out), _ptr(hist), _stream()))
        return out, hist

    def error_mask_hist(self, classes_map, masks, n_classes, out=None):
        """classes_map u8 [B,H,W], masks u8 [B,N,H,W] (non-zero = inside) -> i32 [B,N,n_classes]: pixels of mask n per class."""
        B, N = masks.shape[:2]
        assert classes_map.dtype == torch.uint8 and classes_map.is_contiguous() and classes_map.shape == (B, self.H, self.W)
        assert masks.dtype == torch.uint8 and masks.is_contiguous() and masks.shape[2:] == (self.H, self.W)
        if out is None:
            out = torch.empty((B, N, n_classes), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and out.shape == (B, N, n_classes)
        _lib.check(self.lib.quber_error_mask_hist(self.h, _ptr(classes_map), _ptr(masks), B, N, n_classes, _ptr(out), _stream()))
        return out

    def error_score(self, classes_map, explicit, kind, error_type, out=None):
        """classes_map u8 [B,H,W], explicit u8 [B,2,4,H,W] (error_maps()); kind 0 / "region" | 1 / "boundary"; error_type a name
        or index of eval.error_maps.ERROR_TYPES -> confusion table i64 [B,classes+1,classes] (row = target, column = predicted)."""
        from .eval import error_maps as em
        et = em.ERROR_TYPES.index(error_type) if isinstance(error_type, str) else int(error_type)
        kd = ("region", "boundary").index(kind) if isinstance(kind, str) else int(kind)
        ncls = len(em.CLASS_NAMES[em.ERROR_TYPES[et]])
        B = classes_map.shape[0]
        assert classes_map.dtype == torch.uint8 and classes_map.is_contiguous() and classes_map.shape == (B, self.H, self.W)
        assert explicit.dtype == torch.uint8 and explicit.is_contiguous() and explicit.shape == (B, 2, 4, self.H, self.W)
        if out is None:
            out = torch.empty((B, ncls + 1, ncls), dtype=torch.int64, device=self.device)
        assert out.dtype == torch.int64 and out.is_contiguous() and out.shape == (B, ncls + 1, ncls)
        _lib.check(self.lib.quber_error_score(self.h, _ptr(classes_map), _ptr(explicit), kd, et, ncls, B, _ptr(out), _stream()))
        return out

    def error_overlay(self, bgr, classes_map, palette, out=None):
        """bgr u8 [B,H,W,3], classes_map u8 [B,H,W]; palette: up to 4 entries, a (B, G, R) colour or None (class not painted)
        -> u8 [B,H,W,3]; out may be bgr."""
        B = bgr.shape[0]
        assert bgr.dtype == torch.uint8 and bgr.is_contiguous() and bgr.shape == (B, self.H, self.W, 3)
        assert classes_map.dtype == torch.uint8 and classes_map.is_contiguous() and classes_map.shape == (B, self.H, self.W)
        assert len(palette) <= 4
        cols = [0, 0, 0, 0]
        for i, p in enumerate(palette):
            if p is not None:
                cols[i] = (int(p[0]) & 255) | (int(p[1]) & 255) << 8 | (int(p[2]) & 255) << 16 | 1 << 24
        if out is None:
            out = torch.empty_like(bgr)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == bgr.shape
        _lib.check(self.lib.quber_error_overlay(self.h, _ptr(bgr), _ptr(classes_map), B, *cols, _ptr(out), _stream()))
        return out

    # ---- iterative refinement on the device (csrc/iterate.hip; INTEGRATION.md "Iterative refinement") ----
    def relabel_panoptic(self, post, mirror=False, out=None):
        """post: the dict of postprocess() -> compact ids i32 [B,H,W] (0 = no instance, 1 + j = the frame's j-th label), the input of
        encode_label_map().  mirror: [2B,H,W], frames [B,2B) holding the W-mirrors of frames [0,B)."""
        pan = post["panoptic"]
        B = pan.shape[0]
        assert pan.dtype == torch.float32 and pan.is_contiguous() and pan.shape == (B, self.H, self.W)
        assert post["labels"].dtype == torch.float32 and post["labels"].is_contiguous() and post["labels"].shape == (B, self.cap)
        assert post["count"].dtype == torch.int32 and post["count"].shape == (B,)
        shape = ((2 * B) if mirror else B, self.H, self.W)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and out.shape == shape
        _lib.check(self.lib.quber_relabel_panoptic(self.h, _ptr(pan), _ptr(post["labels"]), _ptr(post["count"]), B, int(bool(mirror)),
                                                   _ptr(out), _stream()))
        return out

    def overlap_masks(self, masks, ids, n_ids, out=None):
        """masks u8 [B,N,H,W] (non-zero = inside), ids i32 [B,H,W] in 0..n_ids -> (table i32 [B,N,n_ids+1]: pixels of mask n with
        id j, area i32 [B,n_ids+1]: pixels with id j).  out: a (table, area) pair to write into."""
        B, N = masks.shape[:2]
        assert masks.dtype == torch.uint8 and masks.is_contiguous() and masks.shape[2:] == (self.H, self.W)
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.shape == (B, self.H, self.W)
        table, area = out if out is not None else (None, None)
        if table is None:
            table = torch.empty((B, N, n_ids + 1), dtype=torch.int32, device=self.device)
        if area is None:
            area = torch.empty((B, n_ids + 1), dtype=torch.int32, device=self.device)
        assert table.dtype == torch.int32 and table.is_contiguous() and table.shape == (B, N, n_ids + 1)
        assert area.dtype == torch.int32 and area.is_contiguous() and area.shape == (B, n_ids + 1)
        _lib.check(self.lib.quber_overlap_masks(self.h, _ptr(masks), _ptr(ids), B, N, n_ids, _ptr(table), _ptr(area), _stream()))
        return table, area

    def overlap_ids(self, a, b, n_a, n_b, out=None):
        """a, b i32 [B,H,W] with ids in 0..n_a / 0..n_b -> i32 [B,n_a+1,n_b+1]: pixels with a == i and b == j."""
        B = a.shape[0]
        for t in (a, b):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.shape == (B, self.H, self.W)
        if out is None:
            out = torch.empty((B, n_a + 1, n_b + 1), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and out.shape == (B, n_a + 1, n_b + 1)
        _lib.check(self.lib.quber_overlap_ids(self.h, _ptr(a), _ptr(b), B, n_a, n_b, _ptr(out), _stream()))
        return out

    # ---- connected-component clean-up on the device (csrc/cleanup.hip; INTEGRATION.md "Connected-component clean-up") ----
    def cleanup_ids(self, ids, n_ids, opts, report=None):
        """ids i32 [B,H,W] in 0..n_ids (device), cleaned IN PLACE under `opts` (a Cleanup, "largest" or "holes") -> (ids, report i32
        [B,n_ids+1,4]: per id the components found, pixels removed, pixels gained, final area; row 0: void components examined, 0,
        pixels filled, final void area)."""
        opts = Cleanup.parse(opts)
        if opts is None:
            raise ValueError("cleanup_ids needs clean-up options")
        B = ids.shape[0]
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.shape == (B, self.H, self.W)
        if report is None:
            report = torch.empty((B, n_ids + 1, 4), dtype=torch.int32, device=self.device)
        assert report.dtype == torch.int32 and report.is_contiguous() and report.shape == (B, n_ids + 1, 4)
        _lib.check(self.lib.quber_cleanup_ids(self.h, _ptr(ids), B, n_ids, *opts.args(), _ptr(report), _stream()))
        return ids, report

    def cleanup_post(self, logits, post, opts, out=None):
        """The clean-up on the tables of postprocess(), in place: post["panoptic"] loses the removed pixels (-1) and gains the filled
        ones, post["scores"] / post["boxes"] are recomputed over the cleaned masks; labels, count and centres stay.  No host read.
        -> report i32 [B,cap+1,4] (row 1 + j: the frame's j-th label); out: a tensor to write it into."""
        opts = Cleanup.parse(opts)
        if opts is None:
            raise ValueError("cleanup_post needs clean-up options")
        B, planes = logits.shape[:2]
        assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.shape[2:] == (self.H, self.W)
        pan = post["panoptic"]
        assert pan.dtype == torch.float32 and pan.is_contiguous() and pan.shape == (B, self.H, self.W)
        for key, shape in (("labels", (B, self.cap)), ("scores", (B, self.cap)), ("boxes", (B, self.cap, 4))):
            assert post[key].dtype == torch.float32 and post[key].is_contiguous() and post[key].shape == shape, key
        assert post["count"].dtype == torch.int32 and post["count"].shape == (B,)
        if out is None:
            out = torch.empty((B, self.cap + 1, 4), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and out.shape == (B, self.cap + 1, 4)
        _lib.check(self.lib.quber_cleanup_postprocess(self.h, _ptr(logits), planes, B, _ptr(pan), _ptr(post["labels"]), _ptr(post["count"]),
                                                      _ptr(post["scores"]), _ptr(post["boxes"]), *opts.args(), _ptr(out), _stream()))
        return out

    # ---- perturbed initial masks on the device (csrc/perturb.hip; INTEGRATION.md "Perturbed initial masks") ----
    def perturb_masks(self, masks, programs, targets, out=None, report=None, placement=0):
        """masks u8 [B,N,H,W], programs i32 [B,N,n_ops,8] (perturb.perturb_program; four operations per round), targets f64 [B,N], all on
        the device -> (perturbed masks u8 [B,N,H,W] of 0 / 255, report i32 [B,N,4]: rounds executed, |seg & g|, |seg | g|, |seg|).
        `out` must not overlap `masks`.  placement: 0 auto, 1 the bit planes in LDS (an error when the frame does not fit), 2 in device
        memory (allocated by the first call that needs it: that call cannot be captured into a graph)."""
        from .perturb import OPS_PER_ROUND
        B, N = masks.shape[:2]
        assert masks.dtype == torch.uint8 and masks.is_contiguous() and masks.shape == (B, N, self.H, self.W)
        assert programs.dtype == torch.int32 and programs.is_contiguous() and programs.dim() == 4 and programs.shape[:2] == (B, N) and programs.shape[3] == 8
        assert targets.dtype == torch.float64 and targets.is_contiguous() and targets.shape == (B, N)
        if out is None:
            out = torch.empty_like(masks)
        if report is None:
            report = torch.empty((B, N, 4), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == masks.shape
        assert report.dtype == torch.int32 and report.is_contiguous() and report.shape == (B, N, 4)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_perturb_masks(self.h, _ptr(masks), B, N, _ptr(programs), programs.shape[2], OPS_PER_ROUND, _ptr(targets),
                                                    _ptr(out), _ptr(report), int(placement), _stream()))
        return out, report

    # ---- mask NMS of scored, overlapping initial masks (csrc/masknms.hip; INTEGRATION.md "Overlapping initial masks") ----
    def mask_nms(self, masks, scores, nms=None, out=None, ids=None, source=None, out_scores=None, report=None):
        """masks u8 [B,N,H,W] (non-zero = inside), scores f32 [B,N] (finite), both on the device; nms: a masknms.MaskNMS (default: the
        reference's, IoU 0.7, large on top) -> {"masks": u8 [B,N,H,W] of 0 / 255, disjoint, compacted to the front; "ids": i32 [B,H,W]
        (0, 1..count); "source": i32 [B,N] (input index, -1 behind count); "scores": f32 [B,N]; "report": i32 [B,4] (count, kept, 0, 0)}.
        `out` may be `masks` itself.  N <= min(max_instances, 1024).  Nothing is copied to the host; the first call on an engine
        allocates the workspace and cannot be captured into a graph."""
        from .masknms import MaskNMS
        nms = MaskNMS() if nms is None else nms
        B, N = masks.shape[:2]
        dev = self.device
        assert masks.dtype == torch.uint8 and masks.is_contiguous() and masks.shape == (B, N, self.H, self.W)
        assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.shape == (B, N)
        out = torch.empty_like(masks) if out is None else out
        ids = torch.empty((B, self.H, self.W), dtype=torch.int32, device=dev) if ids is None else ids
        source = torch.empty((B, N), dtype=torch.int32, device=dev) if source is None else source
        out_scores = torch.empty((B, N), dtype=torch.float32, device=dev) if out_scores is None else out_scores
        report = torch.empty((B, 4), dtype=torch.int32, device=dev) if report is None else report
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == masks.shape
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.shape == (B, self.H, self.W)
        assert source.dtype == torch.int32 and source.is_contiguous() and source.shape == (B, N)
        assert out_scores.dtype == torch.float32 and out_scores.is_contiguous() and out_scores.shape == (B, N)
        assert report.dtype == torch.int32 and report.is_contiguous() and report.shape == (B, 4)
        thresh, on_top = nms.args()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_mask_nms(self.h, _ptr(masks), _ptr(scores), B, N, thresh, on_top, _ptr(out), _ptr(ids), _ptr(source),
                                               _ptr(out_scores), _ptr(report), _stream()))
        return {"masks": out, "ids": ids, "source": source, "scores": out_scores, "report": report}

    # ---- the boundary of masks as Boundary AP takes it (csrc/boundaryap.hip; INTEGRATION.md "Boundary AP") ----
    def mask_boundary(self, masks, dilation, out=None, area=None):
        """masks u8 [n,H,W] on the device (non-zero = inside; any frame size) -> (boundary u8 [n,H,W] of 0 / 1 = m & ~erode_d(m), d =
        dilation in 1..64, zeros outside the frame; area i32 [n,2] = pixels of the mask, pixels of its boundary).  `out` may be `masks`
        itself.  Nothing is copied to the host; a call that needs a larger workspace allocates and cannot be captured into a graph."""
        assert masks.dtype == torch.uint8 and masks.is_contiguous() and masks.dim() == 3
        n, h, w = masks.shape
        out = torch.empty_like(masks) if out is None else out
        area = torch.empty((n, 2), dtype=torch.int32, device=self.device) if area is None else area
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == masks.shape
        assert area.dtype == torch.int32 and area.is_contiguous() and area.shape == (n, 2)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_op_mask_boundary(self.h, _ptr(masks), n, h, w, int(dilation), _ptr(out), _ptr(area), _stream()))
        return out, area

    # ---- scene-level perturbation of a frame's instance list (csrc/scene.hip; INTEGRATION.md "Scene-level perturbation") ----
    def scene_perturb(self, gt, props, n_gt, n_prop, draws, max_masks, min_mask_ratio=0.01, out=None, info=None, report=None):
        """gt u8 [B,N,H,W], props u8 [B,P,H,W] (non-zero = inside; N or P may be 0), n_gt / n_prop i32 [B]: the rows of each frame that
        exist, draws: the tables of scene.ScenePerturb.draws() / scene.scene_draws() as device tensors (fp_act, gs_act u8 [B,P];
        merge_act, split_act, delete_act u8 [B,M]; split_try i32 [B,M,10,4]), all on the device -> {"masks": u8 [B,M,H,W] of 0 / 255,
        zero planes behind count; "info": i32 [B,M,4] (kind, source, members, split); "report": i32 [B,8] (count, n_fp, n_gs, ground
        truths kept, absorbed, splits, deleted, dropped)}.  N + P <= 256, M = max_masks <= 256.  Nothing is copied to the host; the
        first call on an engine (and one that needs a larger workspace) allocates and cannot be captured into a graph."""
        B, N, P, M, dev = gt.shape[0], gt.shape[1], props.shape[1], int(max_masks), self.device
        assert gt.dtype == torch.uint8 and gt.is_contiguous() and gt.shape == (B, N, self.H, self.W)
        assert props.dtype == torch.uint8 and props.is_contiguous() and props.shape == (B, P, self.H, self.W)
        for t in (n_gt, n_prop):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.shape == (B,)
        for key, shape, dtype in (("fp_act", (B, P), torch.uint8), ("gs_act", (B, P), torch.uint8), ("merge_act", (B, M), torch.uint8),
                                  ("split_act", (B, M), torch.uint8), ("delete_act", (B, M), torch.uint8), ("split_try", (B, M, 10, 4), torch.int32)):
            t = draws[key]
            assert t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape and t.device == gt.device, key
        out = torch.empty((B, M, self.H, self.W), dtype=torch.uint8, device=dev) if out is None else out
        info = torch.empty((B, M, 4), dtype=torch.int32, device=dev) if info is None else info
        report = torch.empty((B, 8), dtype=torch.int32, device=dev) if report is None else report
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == (B, M, self.H, self.W)
        assert info.dtype == torch.int32 and info.is_contiguous() and info.shape == (B, M, 4)
        assert report.dtype == torch.int32 and report.is_contiguous() and report.shape == (B, 8)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_scene_perturb(self.h, _ptr(gt) if N else None, _ptr(props) if P else None, _ptr(n_gt), _ptr(n_prop), B, N, P, M,
                                                    float(min_mask_ratio), _ptr(draws["fp_act"]) if P else None, _ptr(draws["gs_act"]) if P else None,
                                                    _ptr(draws["merge_act"]), _ptr(draws["split_act"]), _ptr(draws["split_try"]),
                                                    _ptr(draws["delete_act"]), _ptr(out), _ptr(info), _ptr(report), _stream()))
        return {"masks": out, "info": info, "report": report}

    # ---- mean-shift clustering of pixel embeddings (csrc/meanshift.hip; INTEGRATION.md "Initial masks from pixel embeddings") ----
    def _ms_tensor(self, t, dtype, shape, what):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        assert t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape), what
        return t

    def _ms_emb(self, emb):
        assert emb.dtype == torch.float32 and emb.is_contiguous() and emb.dim() == 4 and emb.shape[2:] == (self.H, self.W)
        return emb.shape[0], emb.shape[1]

    def meanshift_seeds(self, emb, first, num_seeds=100, out=None):
        """emb f32 [B,64,H,W], first i32 [B] (device) -> indices i32 [B,num_seeds]: the seeds picked farthest-first from `first`."""
        B, C = self._ms_emb(emb)
        assert first.dtype == torch.int32 and first.is_contiguous() and first.shape == (B,)
        out = self._ms_tensor(out, torch.int32, (B, int(num_seeds)), "indices")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_meanshift_seeds(self.h, _ptr(emb), B, C, _ptr(first), int(num_seeds), _ptr(out), _stream()))
        return out

    def meanshift_climb(self, emb, seeds=None, indices=None, kappa=20.0, iters=10):
        """emb f32 [B,64,H,W]; seeds f32 [B,S,64] climbed IN PLACE, or indices i32 [B,S]: the pixels to start from (then seeds may be
        None or the tensor to write into) -> seeds: `iters` rounds of Z = normalize(exp(kappa Z X^T) X)."""
        B, C = self._ms_emb(emb)
        assert seeds is not None or indices is not None
        S = indices.shape[1] if indices is not None else seeds.shape[1]
        assert indices is None or (indices.dtype == torch.int32 and indices.is_contiguous() and indices.shape == (B, S))
        seeds = self._ms_tensor(seeds, torch.float32, (B, S, 64), "seeds")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_meanshift_climb(self.h, _ptr(emb), B, C, _ptr(indices), S, float(kappa), int(iters), _ptr(seeds), _stream()))
        return seeds

    def meanshift_link(self, seeds, epsilon=0.04, out=None):
        """seeds f32 [B,S,64] -> seed labels i32 [B,S]: the reference's connected_components over the seeds."""
        B, S = seeds.shape[:2]
        assert seeds.dtype == torch.float32 and seeds.is_contiguous() and seeds.shape == (B, S, 64)
        out = self._ms_tensor(out, torch.int32, (B, S), "seed labels")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_meanshift_link(self.h, _ptr(seeds), B, S, float(epsilon), _ptr(out), _stream()))
        return out

    def meanshift_assign(self, emb, seeds, seed_labels, n_masks, depth_z=None, depth_threshold=None, ids=None, masks=None, report=None):
        """Every pixel to its nearest seed's label, the largest cluster to 0, the depth filter (depth_z f32 [B,H,W] and a threshold, or
        neither), the survivors numbered 1..count -> {"ids": i32 [B,H,W], "masks": u8 [B,n_masks,H,W] of 0 / 255, "report": i32 [B,4] =
        count, clusters before the filter, dropped by depth, truncated}."""
        B, C = self._ms_emb(emb)
        S, N = seeds.shape[1], int(n_masks)
        assert seeds.dtype == torch.float32 and seeds.is_contiguous() and seeds.shape == (B, S, 64)
        assert seed_labels.dtype == torch.int32 and seed_labels.is_contiguous() and seed_labels.shape == (B, S)
        assert (depth_z is None) == (depth_threshold is None), "the depth filter needs both the plane and the threshold"
        assert depth_z is None or (depth_z.dtype == torch.float32 and depth_z.is_contiguous() and depth_z.shape == (B, self.H, self.W))
        ids = self._ms_tensor(ids, torch.int32, (B, self.H, self.W), "ids")
        masks = self._ms_tensor(masks, torch.uint8, (B, N, self.H, self.W), "masks")
        report = self._ms_tensor(report, torch.int32, (B, 4), "report")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_meanshift_assign(self.h, _ptr(emb), B, C, _ptr(seeds), _ptr(seed_labels), S, _ptr(depth_z),
                                                       float(depth_threshold or 0.0), N, _ptr(ids), _ptr(masks) if N else None, _ptr(report),
                                                       _stream()))
        return {"ids": ids, "masks": masks, "report": report}

    def meanshift(self, emb, first, ms=None, n_masks=None, depth_z=None, out=None):
        """The chain seeds -> climb -> link -> assign under `ms` (a meanshift.MeanShift; default: the reference's): emb f32 [B,64,H,W],
        first i32 [B], depth_z f32 [B,H,W] (read only when ms.depth_threshold is set) -> {"indices": i32 [B,S], "seeds": f32 [B,S,64],
        "seed_labels": i32 [B,S], "ids", "masks", "report" as meanshift_assign}.  out: such a dict to write into.  Nothing is copied to
        the host; the first call on an engine allocates the workspace and cannot be captured into a graph."""
        from .meanshift import MeanShift
        ms = MeanShift() if ms is None else ms
        B, C = self._ms_emb(emb)
        S = ms.num_seeds
        N = min(self.cap, 254) if n_masks is None else int(n_masks)
        assert first.dtype == torch.int32 and first.is_contiguous() and first.shape == (B,)
        if ms.depth_threshold is None:
            depth_z = None
        elif depth_z is None:
            raise ValueError("cluster: depth_z is required when depth_threshold is set")
        assert depth_z is None or (depth_z.dtype == torch.float32 and depth_z.is_contiguous() and depth_z.shape == (B, self.H, self.W))
        o = dict(out or {})
        o["indices"] = self._ms_tensor(o.get("indices"), torch.int32, (B, S), "indices")
        o["seeds"] = self._ms_tensor(o.get("seeds"), torch.float32, (B, S, 64), "seeds")
        o["seed_labels"] = self._ms_tensor(o.get("seed_labels"), torch.int32, (B, S), "seed labels")
        o["ids"] = self._ms_tensor(o.get("ids"), torch.int32, (B, self.H, self.W), "ids")
        o["masks"] = self._ms_tensor(o.get("masks"), torch.uint8, (B, N, self.H, self.W), "masks")
        o["report"] = self._ms_tensor(o.get("report"), torch.int32, (B, 4), "report")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_meanshift_cluster(self.h, _ptr(emb), B, C, _ptr(first), S, ms.kappa, ms.iters, ms.epsilon, _ptr(depth_z),
                                                        float(ms.depth_threshold or 0.0), N, _ptr(o["indices"]), _ptr(o["seeds"]),
                                                        _ptr(o["seed_labels"]), _ptr(o["ids"]), _ptr(o["masks"]) if N else None, _ptr(o["report"]),
                                                        _stream()))
        return o

    # ---- Gaussian mean shift of centre votes, and the IMP (csrc/gms.hip; INTEGRATION.md "Initial masks from centre votes") ----
    def _gms_in(self, votes, fg):
        assert votes.dtype == torch.float32 and votes.is_contiguous() and votes.dim() == 4 and votes.shape[1:] == (3, self.H, self.W)
        B = votes.shape[0]
        assert fg.dtype in (torch.uint8, torch.bool) and fg.is_contiguous() and fg.shape == (B, self.H, self.W)
        return B

    def gms_seeds(self, votes, fg, first, draws, subsample=5, out=None, info=None):
        """votes f32 [B,3,H,W], fg u8 / bool [B,H,W], first i32 [B], draws i32 [B,num_seeds]: the bit patterns of the 32-bit draws of
        gms.GaussianMeanShift.draws (``torch.from_numpy(r.view(np.int32))``) -> (indices i32 [B,num_seeds] into the subsampled foreground points, -1 behind
        the frame's seeds; info i32 [B,3] = n, n_sub, seeds of the frame)."""
        B = self._gms_in(votes, fg)
        assert draws.dtype == torch.int32 and draws.is_contiguous() and draws.dim() == 2 and draws.shape[0] == B
        S = draws.shape[1]
        assert first.dtype == torch.int32 and first.is_contiguous() and first.shape == (B,)
        out = self._ms_tensor(out, torch.int32, (B, S), "indices")
        info = self._ms_tensor(info, torch.int32, (B, 3), "info")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_gms_seeds(self.h, _ptr(votes), _ptr(fg), B, int(subsample), _ptr(first), _ptr(draws), S, _ptr(out),
                                                _ptr(info), _stream()))
        return out, info

    def gms_climb(self, votes, fg, seeds=None, indices=None, info=None, sigma=0.02, iters=10, subsample=5):
        """seeds f32 [B,S,3] climbed IN PLACE, or indices i32 [B,S]: the subsampled points to start from (then seeds may be None or the
        tensor to write into); info i32 [B,3] or None (every row is a seed) -> seeds: `iters` rounds of the Gaussian mean shift."""
        B = self._gms_in(votes, fg)
        assert seeds is not None or indices is not None
        S = indices.shape[1] if indices is not None else seeds.shape[1]
        assert indices is None or (indices.dtype == torch.int32 and indices.is_contiguous() and indices.shape == (B, S))
        assert info is None or (info.dtype == torch.int32 and info.is_contiguous() and info.shape == (B, 3))
        seeds = self._ms_tensor(seeds, torch.float32, (B, S, 3), "seeds")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_gms_climb(self.h, _ptr(votes), _ptr(fg), B, int(subsample), _ptr(indices), _ptr(info), S, float(sigma),
                                                int(iters), _ptr(seeds), _stream()))
        return seeds

    def gms_link(self, seeds, info=None, epsilon=0.05, out=None):
        """seeds f32 [B,S,3] -> seed labels i32 [B,S] (-1 behind the frame's seeds): the reference's connected_components."""
        B, S = seeds.shape[:2]
        assert seeds.dtype == torch.float32 and seeds.is_contiguous() and seeds.shape == (B, S, 3)
        assert info is None or (info.dtype == torch.int32 and info.is_contiguous() and info.shape == (B, 3))
        out = self._ms_tensor(out, torch.int32, (B, S), "seed labels")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_gms_link(self.h, _ptr(seeds), B, S, _ptr(info), float(epsilon), _ptr(out), _stream()))
        return out

    def gms_assign(self, votes, fg, seeds, seed_labels, n_masks, info=None, min_pixels=300, ids=None, masks=None, centers=None, report=None):
        """Every foreground pixel to its nearest seed's label, the min_pixels filter, the survivors numbered 1..count -> {"ids": i32
        [B,H,W], "masks": u8 [B,n_masks,H,W] of 0 / 255, "centers": f32 [B,n_masks,3], "report": i32 [B,6] = count, clusters found,
        dropped by min_pixels, truncated, 0, fg pixels}."""
        B = self._gms_in(votes, fg)
        S, N = seeds.shape[1], int(n_masks)
        assert seeds.dtype == torch.float32 and seeds.is_contiguous() and seeds.shape == (B, S, 3)
        assert seed_labels.dtype == torch.int32 and seed_labels.is_contiguous() and seed_labels.shape == (B, S)
        assert info is None or (info.dtype == torch.int32 and info.is_contiguous() and info.shape == (B, 3))
        ids = self._ms_tensor(ids, torch.int32, (B, self.H, self.W), "ids")
        masks = self._ms_tensor(masks, torch.uint8, (B, N, self.H, self.W), "masks")
        centers = self._ms_tensor(centers, torch.float32, (B, N, 3), "centers")
        report = self._ms_tensor(report, torch.int32, (B, 6), "report")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_gms_assign(self.h, _ptr(votes), _ptr(fg), B, _ptr(seeds), _ptr(seed_labels), _ptr(info), S, int(min_pixels),
                                                 N, _ptr(ids), _ptr(masks), _ptr(centers), _ptr(report), _stream()))
        return {"ids": ids, "masks": masks, "centers": centers, "report": report}

    def _gms_imp_fits(self):
        from .gms import IMP_LDS_BYTES, imp_plane_bytes
        if imp_plane_bytes(self.H, self.W) > IMP_LDS_BYTES:
            raise ValueError(f"cluster: the IMP's two bit planes of a {self.H} x {self.W} frame ({imp_plane_bytes(self.H, self.W)} bytes) "
                             f"do not fit the LDS ({IMP_LDS_BYTES}); there is no global-memory fallback")

    def gms_imp(self, ids, n_ids, imp=None, n_masks=0, masks=None, centers=None, report=None):
        """ids i32 [B,H,W] (0, 1..n_ids), processed IN PLACE under `imp` (a gms.IMP; default the reference's): every id opened and closed
        in ascending order on the current map, the largest 4-connected component, empty ids dropped and the rest renumbered ->
        {"ids", "masks": u8 [B,n_masks,H,W] or None, "centers": the given f32 [B,n_ids,3] compacted alike or None, "report": i32 [B,6],
        entries 0 (ids left) and 4 (ids emptied) written}."""
        from .gms import IMP
        imp = IMP() if imp is None else imp
        self._gms_imp_fits()
        B, N = ids.shape[0], int(n_masks)
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.shape == (B, self.H, self.W)
        assert centers is None or (centers.dtype == torch.float32 and centers.is_contiguous() and centers.shape == (B, int(n_ids), 3))
        if N:
            masks = self._ms_tensor(masks, torch.uint8, (B, N, self.H, self.W), "masks")
        report = torch.zeros((B, 6), dtype=torch.int32, device=self.device) if report is None else report
        assert report.dtype == torch.int32 and report.is_contiguous() and report.shape == (B, 6)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_gms_imp(self.h, _ptr(ids), B, int(n_ids), imp.ksize, int(imp.largest), N, _ptr(masks) if N else None,
                                              _ptr(centers), _ptr(report), _stream()))
        return {"ids": ids, "masks": masks if N else None, "centers": centers, "report": report}

    def gms(self, votes, fg, first, draws, gms=None, n_masks=None, out=None):
        """The chain seeds -> climb -> link -> assign -> IMP under `gms` (a gms.GaussianMeanShift; default: the reference's): votes f32
        [B,3,H,W], fg u8 / bool [B,H,W], first i32 [B], draws i32 [B,num_seeds] (32-bit words) -> {"indices": i32 [B,S], "seeds": f32
        [B,S,3], "seed_labels": i32 [B,S], "info": i32 [B,3], "raw_ids": i32 [B,H,W] (before the IMP), "ids", "masks": u8
        [B,n_masks,H,W], "centers": f32 [B,n_masks,3], "report": i32 [B,6]}.  out: such a dict to write into.  Nothing is copied to the
        host; the first call on an engine allocates the workspace and cannot be captured into a graph."""
        from .gms import GaussianMeanShift
        g = GaussianMeanShift() if gms is None else gms
        B = self._gms_in(votes, fg)
        S = g.num_seeds
        N = min(self.cap, 254) if n_masks is None else int(n_masks)
        if g.imp is not None:
            self._gms_imp_fits()
        assert first.dtype == torch.int32 and first.is_contiguous() and first.shape == (B,)
        assert draws.dtype == torch.int32 and draws.is_contiguous() and draws.shape == (B, S)
        o = dict(out or {})
        for key, dtype, shape in (("indices", torch.int32, (B, S)), ("seeds", torch.float32, (B, S, 3)), ("seed_labels", torch.int32, (B, S)),
                                  ("info", torch.int32, (B, 3)), ("raw_ids", torch.int32, (B, self.H, self.W)),
                                  ("ids", torch.int32, (B, self.H, self.W)), ("masks", torch.uint8, (B, N, self.H, self.W)),
                                  ("centers", torch.float32, (B, N, 3)), ("report", torch.int32, (B, 6))):
            o[key] = self._ms_tensor(o.get(key), dtype, shape, key)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_gms_cluster(self.h, _ptr(votes), _ptr(fg), B, _ptr(first), _ptr(draws), S, g.sigma, g.iters, g.epsilon,
                                                  g.subsample, g.min_pixels, g.imp.ksize if g.imp is not None else 0,
                                                  int(g.imp.largest) if g.imp is not None else 0, N, _ptr(o["indices"]), _ptr(o["seeds"]),
                                                  _ptr(o["seed_labels"]), _ptr(o["info"]), _ptr(o["raw_ids"]), _ptr(o["ids"]), _ptr(o["masks"]),
                                                  _ptr(o["centers"]), _ptr(o["report"]), _stream()))
        return o

    # ---- zoom-in refinement: rois, crops, paste (csrc/zoom.hip; INTEGRATION.md "Zoom-in refinement") ----
    def zoom_rois(self, ids, n_ids, padding=0.25, out=None):
        """ids i32 [B,H,W] (device; compact: 0 none, 1..n_ids) -> rois i32 [B,n_ids,4] = (x0, y0, x1, y1) inclusive: the tight extent of
        every id, padded by rint(float32(extent) * padding) per side and clamped to the frame; (0, 0, -1, -1) for an id without a pixel."""
        B = ids.shape[0]
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.shape == (B, self.H, self.W)
        if out is None:
            out = torch.empty((B, n_ids, 4), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.int32 and out.is_contiguous() and out.shape == (B, n_ids, 4)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_zoom_rois(self.h, _ptr(ids), B, int(n_ids), float(padding), _ptr(out), _stream()))
        return out

    def zoom_crop(self, bgr, depth, ids, slots, rois, crop, out=None):
        """bgr (and depth, or None) u8 [B,H,W,3], ids i32 [B,H,W], slots i32 [T,2] = (frame, id), rois i32 [B,n_ids,4], all on the device
        -> (bgr_crop u8 [T,S,S,3], depth_crop likewise or None, mask_crop u8 [T,1,S,S] of 0 / 255), S = crop: the ROI of every slot resized
        bilinearly (align_corners, exact on the bytes), its own mask by the nearest rule.  out: such a triple to write into."""
        B, T, S = ids.shape[0], slots.shape[0], int(crop)
        n_ids = rois.shape[1]
        assert bgr.dtype == torch.uint8 and bgr.is_contiguous() and bgr.shape == (B, self.H, self.W, 3)
        assert depth is None or (depth.dtype == torch.uint8 and depth.is_contiguous() and depth.shape == bgr.shape)
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.shape == (B, self.H, self.W)
        assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.shape == (T, 2)
        assert rois.dtype == torch.int32 and rois.is_contiguous() and rois.shape == (B, n_ids, 4)
        bc, dc, mc = out if out is not None else (None, None, None)
        dev = self.device
        bc = torch.empty((T, S, S, 3), dtype=torch.uint8, device=dev) if bc is None else bc
        dc = (torch.empty((T, S, S, 3), dtype=torch.uint8, device=dev) if dc is None else dc) if depth is not None else None
        mc = torch.empty((T, 1, S, S), dtype=torch.uint8, device=dev) if mc is None else mc
        for t, shape in ((bc, (T, S, S, 3)), (dc, (T, S, S, 3)), (mc, (T, 1, S, S))):
            assert t is None or (t.dtype == torch.uint8 and t.is_contiguous() and t.shape == shape)
        _lib.check(self.lib.quber_zoom_crop(self.h, _ptr(bgr), _ptr(depth), _ptr(ids), _ptr(slots), _ptr(rois), B, n_ids, T, S, _ptr(bc), _ptr(dc),
                                            _ptr(mc), _stream()))
        return bc, dc, mc

    def zoom_paste(self, crop_ids, crop_scores, table, area, depth_crop, slots, rois, batch, min_overlap=0.5, max_inst=254, out=None):
        """crop_ids i32 [T,S,S] (the crop pass's compact ids), crop_scores f32 [T,C], table / area i32 [T,C+1] (overlap_masks of the mask
        crops with crop_ids, on the crop engine), depth_crop u8 [T,S,S,3] or None, slots i32 [T,2] ascending by frame, rois i32 [B,n_ids,4]
        -> {"ids": i32 [B,H,W], "masks": u8 [B,max_inst,H,W] of 0 / 255, "source": i32 [B,max_inst,2] (first-pass id, crop-pass id; -1
        behind count), "scores": f32 [B,max_inst], "boxes": f32 [B,max_inst,4], "report": i32 [B,4] = crops, kept, kept without a final
        id, count}.  out: such a dict to write into.  Nothing is copied to the host."""
        B, T = int(batch), slots.shape[0]
        S = crop_ids.shape[1] if T else 2
        C = crop_scores.shape[1] if T else 1
        n_ids, N, dev = rois.shape[1], int(max_inst), self.device
        if T:
            assert crop_ids.dtype == torch.int32 and crop_ids.is_contiguous() and crop_ids.shape == (T, S, S)
            assert crop_scores.dtype == torch.float32 and crop_scores.is_contiguous() and crop_scores.shape == (T, C)
            for t in (table, area):
                assert t.dtype == torch.int32 and t.is_contiguous() and t.shape == (T, C + 1)
            assert depth_crop is None or (depth_crop.dtype == torch.uint8 and depth_crop.is_contiguous() and depth_crop.shape == (T, S, S, 3))
        assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.shape == (T, 2)
        assert rois.dtype == torch.int32 and rois.is_contiguous() and rois.shape == (B, n_ids, 4)
        spec = {"ids": ((B, self.H, self.W), torch.int32), "masks": ((B, N, self.H, self.W), torch.uint8), "source": ((B, N, 2), torch.int32),
                "scores": ((B, N), torch.float32), "boxes": ((B, N, 4), torch.float32), "report": ((B, 4), torch.int32)}
        o = {} if out is None else out
        for k, (shape, dt) in spec.items():
            if o.get(k) is None:
                o[k] = torch.empty(shape, dtype=dt, device=dev)
            assert o[k].dtype == dt and o[k].is_contiguous() and o[k].shape == shape, k
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_zoom_paste(self.h, _ptr(crop_ids if T else None), _ptr(crop_scores if T else None), _ptr(table if T else None),
                                                 _ptr(area if T else None), _ptr(depth_crop if T else None), _ptr(slots), _ptr(rois), B, n_ids, T, S, C,
                                                 float(min_overlap), N, _ptr(o["ids"]), _ptr(o["masks"]), _ptr(o["source"]), _ptr(o["scores"]),
                                                 _ptr(o["boxes"]), _ptr(o["report"]), _stream()))
        return o

    # ---- Region Refinement Network: crops in, refined masks back (csrc/rrn.hip; INTEGRATION.md "Refined initial masks of the third family") ----
    def rrn_crop(self, bytes_, ids, slots, rois, table, crop, out=None):
        """bytes_ u8 [B,H,W,3], ids i32 [B,H,W], slots i32 [T,2] = (frame, id), rois i32 [B,n_ids,4] (zoom_rois), table f32 [3,256]
        (region.standardize_table), all on the device -> (rgb_crop f32 [T,3,S,S], mask_crop u8 [T,S,S] of 0 / 1), S = crop: rrn_preprocess -
        the standardised ROI of every slot resized bilinearly (align_corners, float32, every operation rounded), its own mask by the nearest
        rule.  out: such a pair to write into."""
        B, T, S = ids.shape[0], slots.shape[0], int(crop)
        n_ids = rois.shape[1]
        assert bytes_.dtype == torch.uint8 and bytes_.is_contiguous() and bytes_.shape == (B, self.H, self.W, 3)
        assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.shape == (B, self.H, self.W)
        assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.shape == (T, 2)
        assert rois.dtype == torch.int32 and rois.is_contiguous() and rois.shape == (B, n_ids, 4)
        assert table.dtype == torch.float32 and table.is_contiguous() and table.shape == (3, 256)
        rc, mc = out if out is not None else (None, None)
        rc = torch.empty((T, 3, S, S), dtype=torch.float32, device=self.device) if rc is None else rc
        mc = torch.empty((T, S, S), dtype=torch.uint8, device=self.device) if mc is None else mc
        assert rc.dtype == torch.float32 and rc.is_contiguous() and rc.shape == (T, 3, S, S)
        assert mc.dtype == torch.uint8 and mc.is_contiguous() and mc.shape == (T, S, S)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_rrn_crop(self.h, _ptr(bytes_), _ptr(ids), _ptr(slots), _ptr(rois), _ptr(table), B, n_ids, T, S, _ptr(rc), _ptr(mc),
                                               _stream()))
        return rc, mc

    def rrn_paste(self, refined, slots, rois, z, batch, n_masks, out=None):
        """refined u8 [T,S,S] (non-zero = foreground), slots i32 [T,2] ascending by frame, rois i32 [B,n_ids,4], z f32 [B,H,W] (NaN counts as 0)
        -> {"ids": i32 [B,H,W], "masks": u8 [B,n_masks,H,W] of 0 / 255, "source": i32 [B,n_masks] (the initial id of each refined mask, 0
        behind the count), "keys": f32 [T] (mean z under each resized mask), "report": i32 [B,4] = refined masks, initial masks that
        vanished, pixels painted, pixels painted over}: rrn_postprocess, ids compacted in ascending order.  out: such a dict to write
        into.  Nothing is copied to the host; the first call on an engine allocates the workspace and cannot be captured into a graph."""
        B, T, N = int(batch), slots.shape[0], int(n_masks)
        S = refined.shape[1] if T else 2
        n_ids, dev = rois.shape[1], self.device
        if T:
            assert refined.dtype == torch.uint8 and refined.is_contiguous() and refined.shape == (T, S, S)
        assert slots.dtype == torch.int32 and slots.is_contiguous() and slots.shape == (T, 2)
        assert rois.dtype == torch.int32 and rois.is_contiguous() and rois.shape == (B, n_ids, 4)
        assert z.dtype == torch.float32 and z.is_contiguous() and z.shape == (B, self.H, self.W)
        spec = {"ids": ((B, self.H, self.W), torch.int32), "masks": ((B, N, self.H, self.W), torch.uint8), "source": ((B, N), torch.int32),
                "keys": ((T,), torch.float32), "report": ((B, 4), torch.int32)}
        o = {} if out is None else out
        for k, (shape, dt) in spec.items():
            if o.get(k) is None:
                o[k] = torch.empty(shape, dtype=dt, device=dev)
            assert o[k].dtype == dt and o[k].is_contiguous() and o[k].shape == shape, k
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_rrn_paste(self.h, _ptr(refined if T else None), _ptr(slots if T else None), _ptr(rois if T else None), _ptr(z), B,
                                                n_ids, T, S, N, _ptr(o["ids"]), _ptr(o["masks"]), _ptr(o["source"]), _ptr(o["keys"] if T else None),
                                                _ptr(o["report"]), _stream()))
        return o

    # ---- validation losses: training targets, loss record (csrc/losses.hip; INTEGRATION.md "Validation losses") ----
    def loss_targets(self, gt_labels, n_gt, spec=None, out=None):
        """gt_labels i32 [B,H,W] (device; 0 = none, 1..n_gt, anything else counts as 0), spec: a losses.Losses (default: the reference's
        sigma 10, small area 4096, weight 3) -> {"targets": f32 [B,6,H,W] (losses.TARGET_PLANES: centre heat, off_y, off_x, sem_seg,
        sem_seg_weights, inst_weights), "points": f64 [B,n_gt,2] (cy, cx), "area": i32 [B,n_gt]}; zeros for an id without a pixel.  out:
        such a dict to write into.  Nothing is copied to the host; the first call of loss_targets / losses on an engine allocates their
        workspace and cannot be captured into a graph."""
        from . import losses as ls
        spec = ls.Losses() if spec is None else spec
        B, n, dev = gt_labels.shape[0], int(n_gt), self.device
        assert gt_labels.dtype == torch.int32 and gt_labels.is_contiguous() and gt_labels.shape == (B, self.H, self.W)
        key = ("loss_gauss", spec.sigma)
        cache = self.__dict__.setdefault("_loss_gauss", {})
        if key not in cache:
            cache[key] = torch.from_numpy(ls.gauss_table(spec.sigma).copy()).to(dev)
        shapes = {"targets": ((B, 6, self.H, self.W), torch.float32), "points": ((B, n, 2), torch.float64), "area": ((B, n), torch.int32)}
        o = {} if out is None else out
        for k, (shape, dt) in shapes.items():
            if o.get(k) is None:
                o[k] = torch.empty(shape, dtype=dt, device=dev)
            assert o[k].dtype == dt and o[k].is_contiguous() and o[k].shape == shape, k
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_loss_targets(self.h, _ptr(gt_labels), B, n, spec.sigma, spec.small_area, float(spec.small_weight),
                                                   _ptr(cache[key]), _ptr(o["targets"]), _ptr(o["points"] if n else None),
                                                   _ptr(o["area"] if n else None), _stream()))
        return o

    def loss_heads(self, spec):
        """{head name: first logit plane} of the engine's error heads, for `spec`'s error type."""
        from . import losses as ls
        heads = {k: first for k, (first, _) in self.error_heads().items()}
        if heads and ls.ERROR_CLASSES[spec.error_type] != self.qcfg.error_classes:
            raise ValueError(f"losses: error_type {spec.error_type!r} has {ls.ERROR_CLASSES[spec.error_type]} classes, the engine's error heads "
                             f"{self.qcfg.error_classes}")
        return heads

    def losses(self, logits, targets, explicit, spec=None, out=None, heads=None):
        """logits f32 [B,P,H,W], targets f32 [B,6,H,W] (loss_targets()["targets"]), explicit u8 [B,2,4,H,W] (error_maps()) or None, all on the
        device; spec: a losses.Losses; heads: {"eee_mask" | "eee_boundary": first logit plane} (default: the engine's error heads when
        `explicit` is given, none otherwise) -> f64 [B,losses.LOSS_WORDS], one record per frame (include/quber_hip.h: quber_losses;
        Losses.unpack reads it).  Nothing is copied to the host."""
        from . import losses as ls
        spec = ls.Losses() if spec is None else spec
        B, P = logits.shape[:2]
        assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.shape[2:] == (self.H, self.W)
        assert targets.dtype == torch.float32 and targets.is_contiguous() and targets.shape == (B, 6, self.H, self.W)
        if heads is None:
            heads = self.loss_heads(spec) if explicit is not None else {}
        if heads:
            assert explicit is not None and explicit.dtype == torch.uint8 and explicit.is_contiguous() and explicit.shape == (B, 2, 4, self.H, self.W)
        spec.top_k_pixels(self.H * self.W)
        if out is None:
            out = torch.empty((B, ls.LOSS_WORDS), dtype=torch.float64, device=self.device)
        assert out.dtype == torch.float64 and out.is_contiguous() and out.shape == (B, ls.LOSS_WORDS)
        cs = spec.c_spec(heads)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.quber_losses(self.h, _ptr(logits), P, _ptr(targets), _ptr(explicit if heads else None), C.byref(cs), B, _ptr(out),
                                             _stream()))
        return out

    def extract_masks(self, post, max_inst, out=None):
        B = post["panoptic"].shape[0]
        if out is None:
            out = torch.empty((B, max_inst, self.H, self.W), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.quber_extract_masks(self.h, _ptr(post["panoptic"]), _ptr(post["labels"]), B, max_inst,
                                                _ptr(out), _stream()))
        return out

    def debug_tensor(self, name, batch):
        """NHWC copy [batch,H,W,C] of a named intermediate of the last forward."""
        p, dims, cs = C.c_void_p(), (C.c_int32 * 4)(), C.c_int32()
        _lib.check(self.lib.quber_debug_tensor(self.h, name.encode(), C.byref(p), C.byref(dims), C.byref(cs)))
        Bm, H, W, Cc = list(dims)
        es = self.lib.quber_debug_tensor_elem_size(self.h, name.encode())       # 2: the fp16 data path stores activations as fp16
        n = (batch * H * W - 1) * cs.value + Cc        # the view may be a channel slice of a wider buffer
        buf = torch.empty(n, dtype=torch.float16 if es == 2 else torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rc = hip.hipMemcpy(C.c_void_p(buf.data_ptr()), p, n * es, 3)
        if rc != 0:
            raise _lib.QuberError(f"hipMemcpy failed ({rc})")
        return torch.as_strided(buf, (batch, H, W, Cc), (H * W * cs.value, W * cs.value, cs.value, 1)).float()
