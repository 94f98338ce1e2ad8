"""The Region Refinement Network of UOIS-Net-3D on the MI355X HIP path (csrc/rrn.hip, csrc/plan_rrn.hip): the initial masks of
``cluster=GaussianMeanShift()`` are cropped, refined by the network and painted back, without leaving the device.

``RrnEngine`` is one context for a fixed crop side and batch capacity; ``RegionRefinement`` the options object of
``MaskRefinerPredictor(..., cluster=GaussianMeanShift.uois(), region=RegionRefinement(weights))``."""
import ctypes as C

import numpy as np
import torch

from .. import _lib, engine as qengine, rrn_arch

RRN_HEAD = 54                  # option key: decoder.last_conv + fg_module as one collapsed 3x3 filter (csrc/rrn.hip rrn_head3) or convolution + 1x1 head
MEAN = (0.485, 0.456, 0.406)   # standardize_image, eval/preprocess_utils.py:82-93
STD = (0.229, 0.224, 0.225)


def standardize_table(mean=MEAN, std=STD):
    """f32 [3,256]: table[c][v] = float32((v / 255. - mean[c]) / std[c]), in float64 exactly as numpy evaluates standardize_image.  Byte
    channel c takes mean[c]: the reference standardises the BGR bytes of cv2.imread with these RGB-ordered means (eval/base_model.py:460-462),
    and so does this table on BGR bytes."""
    v = np.arange(256, dtype=np.float64)
    return np.stack([((v / 255. - mean[c]) / std[c]).astype(np.float32) for c in range(3)])


class RrnEngine:
    """One Region Refinement Network context (quber_config.with_network = 5).  crop: the side S of the square crops, a multiple of 16.
    head: option key 54, None = the library's default.  All methods are asynchronous on torch's current stream and take device tensors."""

    def __init__(self, state_dict, crop=224, max_batch=20, head=None, device="cuda:0"):
        if crop % 16 or crop < 16:
            raise ValueError(f"RrnEngine: the crop side must be a multiple of 16 (got {crop})")
        sd = rrn_arch.load_checkpoint(state_dict)
        self.feature_dim = int(sd[rrn_arch.FIRST].shape[0])
        qc = qengine.make_config(crop, crop, max_batch=max_batch)
        qc.with_network = 5
        self.eng = qengine.Engine(qc, device)
        if head is not None:
            self.eng.set_option(RRN_HEAD, int(bool(head)))
        # the context's inventory names the keys; the sizes follow from feature_dim, which the plan reads off the first convolution
        lib = self.eng.lib
        for name, _ in self.eng.weight_specs():
            v = sd[name]
            _lib.check(lib.quber_set_weight(self.eng.h, name.encode(), C.c_void_p(v.ctypes.data), v.size))
        with torch.cuda.device(self.eng.device):
            _lib.check(lib.quber_finalize_weights(self.eng.h))
        self.device = self.eng.device
        self.S, self.max_batch = crop, max_batch

    def close(self):
        self.eng.close()

    def _check(self, rgb, mask):
        n, S = rgb.shape[0], self.S
        if not (rgb.dtype == torch.float32 and rgb.is_contiguous() and rgb.is_cuda and tuple(rgb.shape) == (n, 3, S, S)):
            raise ValueError(f"RrnEngine: rgb crops must be a contiguous float32 device tensor [n,3,{S},{S}]")
        if not (mask.dtype == torch.uint8 and mask.is_contiguous() and mask.is_cuda and tuple(mask.shape) == (n, S, S)):
            raise ValueError(f"RrnEngine: mask crops must be a contiguous uint8 device tensor [n,{S},{S}]")
        if not 1 <= n <= self.max_batch:
            raise ValueError(f"RrnEngine: {n} crops outside 1..{self.max_batch}")
        return n

    def run(self, rgb, mask, threshold=0.5, logits=True, refined=True, out=None):
        """rgb f32 [n,3,S,S] (standardised), mask u8 [n,S,S] (non-zero = initial mask) -> {"logits": f32 [n,S,S], "refined": u8 [n,S,S] =
        (logit > float32(log(t / (1 - t)))), 0 / 1}, whichever is requested.  out: such a dict to write into."""
        n = self._check(rgb, mask)
        o = {} if out is None else out
        for k, want, dt in (("logits", logits, torch.float32), ("refined", refined, torch.uint8)):
            if want and o.get(k) is None:
                o[k] = torch.empty((n, self.S, self.S), dtype=dt, device=self.device)
            if want:
                assert o[k].dtype == dt and o[k].is_contiguous() and tuple(o[k].shape) == (n, self.S, self.S), k
        p = lambda k, want: C.c_void_p(o[k].data_ptr() if want else 0)
        with torch.cuda.device(self.device):
            _lib.check(self.eng.lib.quber_rrn_forward(self.eng.h, C.c_void_p(rgb.data_ptr()), C.c_void_p(mask.data_ptr()), n,
                                                      C.c_float(float(rrn_arch.logit_threshold(threshold))), p("logits", logits), p("refined", refined),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return {k: o[k] for k, want in (("logits", logits), ("refined", refined)) if want}

    def forward(self, rgb, mask):
        """-> logits f32 [n,S,S]: RegionRefinementNetwork.forward"""
        return self.run(rgb, mask, refined=False)["logits"]

    def profile(self, rgb, mask):
        """One forward with an event pair around every op -> [(op name, ms)] in plan order; synchronises (tools/rrn_ab.py)."""
        n = self._check(rgb, mask)
        plan = self.eng.plan()
        ms = (C.c_double * len(plan))()
        ref = torch.empty((n, self.S, self.S), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.eng.lib.quber_rrn_forward_profiled(self.eng.h, C.c_void_p(rgb.data_ptr()), C.c_void_p(mask.data_ptr()), n, C.c_float(0.0), None,
                                                               C.c_void_p(ref.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream), ms))
        return [(p[0], ms[i]) for i, p in enumerate(plan)]


class RegionRefinement:
    """Options of ``MaskRefinerPredictor(region=...)``: the weights (a state dict, a checkpoint dict with it under 'model', or a path to one;
    DataParallel's ``module.`` prefix is stripped), the ROI padding (``padding_percentage``), the probability threshold, the crop side and
    how many crops go through the network at a time (the reference's step_size: only chunking, GroupNorm is per sample).  head: option key
    54, None = the library's default.  final_close_morphology (uois/src/segmentation.py:545-573, "for synthetically-trained RRN"): after
    the paste every id of the refined map, in ascending order, is opened and then closed with OpenCV's ksize ellipse on the current map -
    a later id paints over an earlier one where their closings meet - and the ids the opening removed are compacted away (the reference's
    np.unique, eval/base_model.py:512).  It is the IMP of ``cluster=`` without the largest-component step, on the same kernel."""

    def __init__(self, weights_or_path, padding=0.25, threshold=0.5, crop=224, chunk=20, head=None, final_close_morphology=False, ksize=9):
        self.state_dict = rrn_arch.load_checkpoint(weights_or_path)
        rrn_arch.logit_threshold(threshold)
        if crop % 16 or crop < 16:
            raise ValueError(f"RegionRefinement: the crop side must be a multiple of 16 (got {crop})")
        if chunk < 1:
            raise ValueError("RegionRefinement: chunk must be at least 1")
        self.padding, self.threshold, self.crop, self.chunk, self.head = float(padding), float(threshold), int(crop), int(chunk), head
        if not isinstance(final_close_morphology, (bool, np.bool_)):
            raise ValueError("RegionRefinement: final_close_morphology must be a bool")
        self.final_close_morphology = bool(final_close_morphology)
        self.close_imp = None
        if self.final_close_morphology:
            from ..gms import IMP
            self.close_imp = IMP(ksize, largest=False)
        self._engines = {}
        self._tables = {}

    def engine_for(self, device):
        key = (self.crop, self.chunk, str(device))
        if key not in self._engines:
            self._engines[key] = RrnEngine(self.state_dict, self.crop, self.chunk, head=self.head, device=device)
        return self._engines[key]

    def table_for(self, device):
        key = str(device)
        if key not in self._tables:
            self._tables[key] = torch.from_numpy(standardize_table()).to(device)
        return self._tables[key]

    def refine(self, eng, bytes_, ids, n_ids, counts, z):
        """The whole stage on the frame engine `eng`: bytes_ u8 [B,H,W,3], ids i32 [B,H,W] (compact, 1..n_ids), counts: the ids present
        per frame (host ints: frame b holds 1..counts[b]), z f32 [B,H,W], all tensors on the device -> the dict of Engine.rrn_paste plus
        "rois", "slots", "refined" (u8 [T,S,S]).  With final_close_morphology "ids", "masks" and "source" are those after the close and
        "report" is i32 [B,5]: the masks left, the initial masks the network emptied, pixels painted, pixels painted over (both by the
        paste), the ids the close removed."""
        B, S = ids.shape[0], self.crop
        rois = eng.zoom_rois(ids, n_ids, self.padding)
        slots = torch.tensor([(b, i) for b in range(B) for i in range(1, int(counts[b]) + 1)], dtype=torch.int32).reshape(-1, 2).to(eng.device)
        T = slots.shape[0]
        refined = torch.empty((T, S, S), dtype=torch.uint8, device=eng.device)
        if T:
            rgb, mask = eng.rrn_crop(bytes_, ids, slots, rois, self.table_for(eng.device), S)
            net = self.engine_for(eng.device)
            for a in range(0, T, self.chunk):
                e = min(T, a + self.chunk)
                net.run(rgb[a:e], mask[a:e], self.threshold, logits=False, out={"refined": refined[a:e]})
        N = max(n_ids, 1)
        o = eng.rrn_paste(refined, slots, rois, z, B, N)
        if self.close_imp is not None:
            # the IMP compacts a [B,N,3] float table beside the ids: it carries the source ids (at most 254: exact in float32) along
            src = o["source"].to(torch.float32)[:, :, None].expand(B, N, 3).contiguous()
            imp = eng.gms_imp(o["ids"], N, self.close_imp, n_masks=N, masks=o["masks"], centers=src)
            o["source"] = src[:, :, 0].to(torch.int32).contiguous()
            o["report"] = torch.cat([imp["report"][:, 0:1], o["report"][:, 1:4], imp["report"][:, 4:5]], 1).contiguous()
        o.update(rois=rois, slots=slots, refined=refined)
        return o

    def close(self):
        for e in self._engines.values():
            e.close()
        self._engines = {}
