"""Drop-in for the reference's ``eval/refiner_model.py:MaskRefiner`` adapter (reference lines 214-297):
``MaskRefiner(config_file, weights_file, dataset).predict(rgb_path, depth_path, initial_masks, fg_mask)
-> (refined_masks bool [K,H,W] | [], output dict, seconds, fg_mask)``.

Built, all on the device: ``cv2.resize`` of the BGR image to 640x480 (INTER_LINEAR, OpenCV's 8-bit fixed-point path,
``quber_resize_u8``), ``normalize_depth`` (eval/preprocess_utils.py:12-28; bit-exact against the imported reference
function), the nearest depth / mask resizes, the HIP predictor, the LMFFNet foreground post-filter (refiner_model.py:
273-277) and the OCID zero-depth masking (refiner_model.py:279-288).  The ``dataset == 'armbench'`` branch
(refiner_model.py:226-244: RGB only, shortest edge 800 / longest 1333, nearest resize of the masks) is built too.

Return semantics follow the reference exactly: the foreground filter decides which masks survive only for
``dataset == 'OCID'`` (refiner_model.py:279-288 is the only place ``filt_masks`` is returned); every other dataset gets
the unfiltered refined masks plus the foreground mask.  The reference always constructs ``lmffNet()``; here the filter
is opt-in (``foreground_filter=True``) because the reference's ``rgbd_lmffnet.pth`` does not ship and seeded weights give
a meaningless foreground - with it off, ``fg_mask`` is None and the OCID branch masks zero depth on the unfiltered masks.

``inpaint_depth`` (eval/preprocess_utils.py:44-64: the pixels whose NORMALISED depth is 0 - holes and everything nearer than
``min_val`` - are filled with ``cv2.inpaint(..., 3, cv2.INPAINT_TELEA)``): ``inpaint="host"`` (default) runs
``quber_inpaint_depth_u8`` (csrc/inpaint.hip: Telea's fast-marching method restated in the form OpenCV implements it; parity with cv2
unpinned, own tolerance - OpenCV is not in the image) on the calling thread, as the reference does; ``inpaint="device"`` runs
csrc/inpaint_dev.hip, which marches the independent hole regions one wave each and equals the host function bit for bit
(tests/test_gpu_inpaint.py).  ``MaskRefiner(inpaint=False)`` skips it.
cv2 / imageio are absent from the image, so files are read with PIL.

``MaskRefinerTTA`` is the refiner the reference's driver builds for ``--refiner_model maskrefiner-tta``
(eval/un_eval_utils.py:78-81) and never defines: ``MaskRefiner`` with horizontal-flip test-time augmentation (``tta=True``; the
definition is in INTEGRATION.md).
"""
import time

import numpy as np
import torch
from PIL import Image

from .. import engine as qengine
from ..masknms import check_scores
from ..maskrefiner.predictor import MaskRefinerPredictor, RefineOptions, mask_bytes

W = 640
H = 480


def normalize_depth(depth, min_val=250.0, max_val=1500.0):
    depth = np.array(depth, dtype=np.float64 if depth.dtype == np.float64 else np.float32)
    depth = np.clip(depth, min_val, max_val)
    depth = (depth - min_val) / (max_val - min_val) * 255
    if depth.ndim == 2:
        depth = depth[..., None]
    return np.uint8(np.repeat(depth, 3, -1))


def inpaint_depth(depth, kernel_size=3):
    """eval/preprocess_utils.py:44-64 with factor = 1: mask = pixels whose three channels are 0, dilated by a 3x3 square;
    TELEA in-painting with radius 3; only the zero pixels of the input are replaced.  One host call (csrc/inpaint.hip:
    inpaint_depth_u8_host) that releases the GIL from the mask preparation to the merge: predict_stream's worker threads run it
    side by side (the numpy form of the mask preparation held the interpreter lock for ~2 ms per frame)."""
    import ctypes as C
    from .. import _lib
    lib = _lib.load()
    depth = np.ascontiguousarray(depth, dtype=np.uint8)
    if depth.ndim != 3 or depth.shape[2] != 3:
        raise ValueError("inpaint_depth expects a [H, W, 3] uint8 depth image")
    h, w = depth.shape[:2]
    out = np.empty_like(depth)
    _lib.check(lib.quber_inpaint_depth_u8(C.c_void_p(depth.ctypes.data), h, w, kernel_size, C.c_void_p(out.ctypes.data)))
    return out


# the annotation labels the reference's evaluation loop treats as background on OCID (eval/eval_utils.py:33-35)
OCID_BG_LABELS = {"floor": (0, 1), "table": (0, 1, 2)}


def load_annotation(anno_path, rgb_path, dataset, resize=None):
    """The annotation of one frame as the reference's loop prepares it (eval/eval_utils.py:240-248): read, nearest resize to 640x480,
    and on OCID the floor / table labels set to 0.  anno_path: a file, or the array already read; resize: cv2.resize's stand-in
    (img u8, h, w, linear) -> img, e.g. MaskRefiner._resize - needed only for an annotation of another size."""
    anno = np.array(anno_path) if isinstance(anno_path, np.ndarray) else np.array(Image.open(anno_path))
    if anno.shape[:2] != (H, W):
        if resize is None:
            raise ValueError(f"annotation of {anno.shape[:2]}: pass resize= (MaskRefiner._resize) to bring it to {(H, W)}")
        if anno.dtype == np.uint8:
            anno = np.array(resize(anno, H, W, False))
        elif anno.ndim == 2:                         # nearest picks whole pixels: the bytes of a wider type go through as channels
            raw = np.ascontiguousarray(anno)
            planes = raw.view(np.uint8).reshape(raw.shape[0], raw.shape[1], raw.dtype.itemsize)
            anno = np.ascontiguousarray(resize(planes, H, W, False)).view(raw.dtype).reshape(H, W)
        else:
            raise ValueError("annotation: only 8-bit images have a multi-channel resize")
    if dataset == "OCID":
        floor_table = "floor" if "floor" in rgb_path else "table" if "table" in rgb_path else None
        if floor_table is None:
            raise ValueError(f"OCID frame {rgb_path!r}: neither a floor nor a table scene")
        for label in OCID_BG_LABELS[floor_table]:
            anno[anno == label] = 0
    return anno


def label_map_from_masks(masks, shape, dtype=np.int32):
    """The label map the reference's loop paints from a list of masks (eval/eval_utils.py:281-286): mask i as i + 1, later masks on top."""
    pred = np.zeros(shape, dtype)
    for i, mask in enumerate(masks):
        pred[np.asarray(mask) > False] = i + 1
    return pred


def compact_labels(anno):
    """An annotation's label image -> i32 ids 0 (label 0: none), 1..n in ascending label order: what gt_labels= takes."""
    values = np.unique(anno)
    values = values[values != 0]
    if len(values) > 254:
        raise ValueError(f"annotation with {len(values)} labels: at most 254")
    return np.searchsorted(values, anno).astype(np.int32) + (anno != 0).astype(np.int32) if len(values) else np.zeros(anno.shape, np.int32)


def mean_losses(frames):
    """[{key: float}] -> {key: mean over the frames that have the key}."""
    keys = sorted({k for f in frames for k in f})
    return {k: float(np.mean([f[k] for f in frames if k in f])) for k in keys}


def resize_shortest_edge_shape(oldh, oldw, short_edge_length=800, max_size=1333):
    """[d2] ResizeShortestEdge.get_output_shape, used by the armbench branch (refiner_model.py:228)."""
    scale = short_edge_length * 1.0 / min(oldh, oldw)
    newh, neww = (short_edge_length, scale * oldw) if oldh < oldw else (scale * oldh, short_edge_length)
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


class MaskRefiner:
    def __init__(self, config_file=None, weights_file=None, dataset="OSD", device="cuda:0", foreground_filter=False,
                 lmffnet_weights="./foreground_segmentation/rgbd_lmffnet.pth", inpaint="host", tta=False,
                 decode_errors=False, iterations=1, until_converged=False, track_initial=False, cleanup=None, perturb=None,
                 nms=None, zoom=None, losses=None, scene=None, initial_filter=None, cluster=None, seeding=None, region=None, camera=None):
        # cluster / seeding / region: the predictor's base-model stages (a GaussianMeanShift, a quber_amd.seeding.DepthSeeding, a
        # quber_amd.region.RegionRefinement).  With seeding= set predict(rgb_path, depth_path) makes its own initial masks: the point cloud
        # comes from the .pcd beside the depth file (quber_amd/eval/base_model.py: the reference's path rules) or, with camera= (a
        # quber_amd.camera.Camera of the 640 x 480 frame), from the depth file itself; they come back as output["cluster_*"] / ["region_*"]
        # initial_filter: None | "cgnet" | a quber_amd.foreground.predictor.CGNet - the UOAIS base model's foreground filter
        # (eval/base_model.py:209-216) applied to initial_masks (and mask_scores) in _load, before anything else reads them:
        # predict() and predict_stream() alike; the foreground map and the kept indices come back as output["initial_fg"] / ["initial_keep"]
        # tta ... scene: the predictor's options (maskrefiner/predictor.py: module docstring, RefineOptions), for predict()
        # and predict_stream(batch=k) alike, except: until_converged stops early in predict() only (the stream always runs the fixed
        # count); cleanup "largest" is the UOIS path's largest_connected_component (4-connected), "holes" the SAM refiner's
        # remove_small_regions(mask, 300, "holes"); nms takes its scores from predict(..., mask_scores=) and a fifth element of
        # predict_stream's items; zoom is predict() only: predict_stream refuses it; losses (a quber_amd.losses.Losses) acts in
        # predict(..., gt_labels=) and validation_losses() - the stream carries no ground truth; scene (a quber_amd.scene.ScenePerturb)
        # takes initial_masks as the frame's ground truth and predict(..., proposals=) as its pool of segments: predict_stream refuses it
        options = RefineOptions.parse(tta=tta, decode_errors=decode_errors, iterations=iterations, until_converged=until_converged,
                                      track_initial=track_initial, cleanup=cleanup, perturb=perturb, nms=nms, zoom=zoom, losses=losses,
                                      scene=scene, cluster=cluster)
        if camera is not None and seeding is None:
            raise ValueError("camera= needs seeding= (a quber_amd.seeding.DepthSeeding)")
        if seeding is not None and dataset == "armbench":
            raise ValueError("seeding: the Depth Seeding Network reads a point cloud; the armbench path has no depth")
        self.camera = camera
        if camera is not None:
            from ..camera import Camera
            if not isinstance(camera, Camera):
                raise ValueError(f"camera={camera!r}: expected None or a quber_amd.camera.Camera")
        self.refiner_predictor = MaskRefinerPredictor(config_file, weights_file=weights_file, device=device, options=options, seeding=seeding,
                                                      region=region)
        self.dataset = dataset
        self.lmffnet = None
        # "host" / True (default): csrc/inpaint.hip on the calling (worker) thread; "device": csrc/inpaint_dev.hip, bit-equal, for hosts
        # short of CPU cores - a march occupies one wave per hole region for milliseconds and, streamed beside the refiner's batches,
        # costs more GPU time than the host cores it frees are worth on this box: 193 against 278 frames/s (profiles/r09f_adapter_stream.txt);
        # False: none
        self.inpaint = "host" if inpaint is True else inpaint
        if foreground_filter:
            from ..foreground.predictor import lmffNet
            self.lmffnet = lmffNet(lmffnet_weights, device=device)
        self.initial_filter = None
        if initial_filter is not None:
            from ..foreground.predictor import CGNet
            if dataset == "armbench":
                raise ValueError("initial_filter: CGNet reads a depth image; the armbench path has none")
            if isinstance(initial_filter, str) and initial_filter != "cgnet":
                raise ValueError(f"initial_filter: unknown filter '{initial_filter}' (None, 'cgnet' or a CGNet instance)")
            self.initial_filter = CGNet(device=device) if isinstance(initial_filter, str) else initial_filter

    def _dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.refiner_predictor.device)

    def _resize(self, img, h, w, linear):
        """cv2.resize(img, (w, h)) on the device; img: numpy u8 [H,W] / [H,W,C]."""
        if img.shape[:2] == (h, w):
            return np.ascontiguousarray(img)
        return qengine.resize_u8(self._dev(img), h, w, linear).cpu().numpy()

    def _load(self, rgb_path, depth_path, initial_masks, mask_scores=None):
        """File reading and the adapter's pre-processing of one frame (eval/refiner_model.py:224-263): everything before the
        reference's timer starts.  Safe to run on a worker thread (predict_stream): its device work goes to a side stream."""
        rgb = np.asarray(Image.open(rgb_path).convert("RGB"))[:, :, ::-1]        # BGR like cv2.imread
        initial_masks = mask_bytes(initial_masks, True)   # a bool mask is 0 / 255 from here on, whatever the options
        scores = None
        if self.refiner_predictor.nms is not None:        # missing or non-finite scores: refused here, before any device work
            scores = check_scores(mask_scores, len(initial_masks))
        if self.dataset == "armbench":
            h, w = resize_shortest_edge_shape(rgb.shape[0], rgb.shape[1], 800, 1333)
            rgb = self._resize(rgb, h, w, linear=True)                           # cv2.resize(rgb_img, (w, h))
            initial_masks = np.array([self._resize(m, h, w, linear=False) for m in initial_masks])   # INTER_NEAREST
            return {"rgb": np.ascontiguousarray(rgb), "depth": None, "masks": initial_masks, "zero_depth": None, "scores": scores}
        depth = np.load(depth_path) if "npy" in depth_path else np.asarray(Image.open(depth_path))
        rgb = self._resize(rgb, H, W, linear=True)                               # cv2.resize(rgb_img, (W, H))
        zero_depth = np.where(depth == 0)
        lo, hi = (0.25, 1.5) if "npy" in depth_path else (250.0, 1500.0)
        # normalise -> nearest resize -> in-paint: on the device from end to end (refiner_model.py:250-255), one copy back for the
        # numpy-in API of the predictor (the batched stream keeps the device tensor)
        if depth.ndim == 2 and depth.dtype in (np.uint16, np.float32):
            d_dev = qengine.normalize_depth(self._dev(np.array(depth)), lo, hi)[0]
        else:
            d_dev = self._dev(normalize_depth(depth, lo, hi))
        if tuple(d_dev.shape[:2]) != (H, W):
            d_dev = qengine.resize_u8(d_dev, H, W, linear=False)                 # cv2.resize(..., INTER_NEAREST)
        if self.inpaint == "device":
            d_dev = qengine.inpaint_depth(d_dev)                                 # refiner_model.py:255, csrc/inpaint_dev.hip
            depth = d_dev.cpu().numpy()
        elif self.inpaint:
            depth = inpaint_depth(d_dev.cpu().numpy())                           # the host function (bit-equal; csrc/inpaint.hip)
            d_dev = None
        else:
            depth = d_dev.cpu().numpy()
        fr = {"rgb": np.ascontiguousarray(rgb), "depth": depth, "masks": initial_masks, "zero_depth": zero_depth, "depth_dev": d_dev,
              "scores": scores}
        if self.initial_filter is not None:
            # eval/base_model.py:209-216 on the frame as the refiner will see it; the masks keep their own size (the count kernel reads the
            # 240 x 320 foreground map at the nearest-neighbour position)
            from ..foreground.predictor import filter_masks_uoais
            fg, counts = self.initial_filter.filter_counts(fr["rgb"], depth, initial_masks)
            kept, keep = filter_masks_uoais(initial_masks, counts)
            fr["masks"] = np.asarray(kept, dtype=initial_masks.dtype).reshape((len(keep),) + tuple(initial_masks.shape[1:]))
            if scores is not None:
                fr["scores"] = scores[keep]
            fr["initial_fg"], fr["initial_keep"] = fg, keep
        return fr

    def _refine(self, fr, gt_labels=None, proposals=None):
        """The reference's timed region and what follows it (eval/refiner_model.py:265-297) on a loaded frame."""
        start = time.time()
        kw = {} if proposals is None else {"proposals": proposals}
        if self.dataset == "armbench":
            output = self.refiner_predictor.predict(fr["rgb"], None, fr["masks"], fr["scores"], gt_labels=gt_labels, **kw)[0]
        else:
            output = self.refiner_predictor.predict(fr["rgb"], fr["depth"], fr["masks"], fr["scores"], gt_labels=gt_labels, **kw)[0]
        refined = output["instances"].to("cpu").pred_masks.numpy() if "instances" in output else []
        return self._finish(fr, output, refined, start)

    def _finish(self, fr, output, refined, start):
        """What follows the refiner call inside and after the reference's timed region (eval/refiner_model.py:273-297): the
        LMFFNet foreground filter, the elapsed time, the OCID zero-depth masking."""
        if self.dataset == "armbench":
            return refined, output, time.time() - start, None
        rgb, depth, zero_depth = fr["rgb"], fr["depth"], fr["zero_depth"]
        if "initial_keep" in fr:
            output["initial_fg"], output["initial_keep"] = fr["initial_fg"], fr["initial_keep"]
        fg, filt = None, refined
        if self.lmffnet is not None:
            from ..foreground.predictor import filter_masks
            m = self._dev(np.ascontiguousarray(refined, dtype=np.uint8)[None]) if len(refined) else None
            fg_t, counts = self.lmffnet.net.foreground(self._dev(rgb[None]), self._dev(depth[None]), m)
            fg = fg_t[0].cpu().numpy().astype(bool)
            if len(refined):
                filt = np.asarray(filter_masks(refined, counts[0]))              # inter / area > 0.3 (refiner_model.py:274-276)
        elapsed = time.time() - start
        if self.dataset == "OCID":
            # refiner_model.py:279-288: only here do the FILTERED masks (minus zero-depth pixels) replace refined_masks
            out = []
            for m in filt:
                m = m.copy()
                m[zero_depth] = False
                out.append(m)
            refined = np.asarray(out)
        return refined, output, elapsed, fg

    def _predict_seeded(self, rgb_path, depth_path, gt_labels=None):
        """seeding=: the whole base-model chain and the refiner in one predictor call; the geometry is read before the timer starts"""
        from .base_model import load_geometry
        fr = self._load(rgb_path, depth_path, np.zeros((0, H, W), np.uint8))
        kind, geo = load_geometry(depth_path, self.dataset, self.camera, H, W)
        kw = {"xyz": geo} if kind == "xyz" else {"depth_z": geo, "camera": self.camera}
        start = time.time()
        output = self.refiner_predictor.predict(fr["rgb"], fr["depth"], gt_labels=gt_labels, **kw)[0]
        refined = output["instances"].to("cpu").pred_masks.numpy() if "instances" in output else []
        return self._finish(fr, output, refined, start)

    def predict(self, rgb_path, depth_path, initial_masks=None, fg_mask=None, mask_scores=None, gt_labels=None, proposals=None):
        # proposals (with scene=): u8 / bool [P,H,W] at the size of initial_masks - the pool the scene perturbation draws false positives
        # and over- / under-segmentations from; may be absent
        # initial_masks=None (with seeding=): the Depth Seeding Network, the clustering and region= make them
        if self.refiner_predictor.seeding is not None:
            if initial_masks is not None or mask_scores is not None or proposals is not None:
                raise ValueError("seeding: the base-model chain makes the initial masks; initial_masks / mask_scores / proposals were given as well")
            return self._predict_seeded(rgb_path, depth_path, gt_labels)
        if initial_masks is None:
            raise ValueError("initial_masks=None needs seeding= (a quber_amd.seeding.DepthSeeding)")
        fr = self._load(rgb_path, depth_path, initial_masks, mask_scores)
        if proposals is not None and self.dataset == "armbench" and len(proposals):
            h, w = fr["rgb"].shape[:2]
            proposals = np.array([self._resize(m, h, w, linear=False) for m in mask_bytes(proposals, True)])
        return self._refine(fr, gt_labels, proposals)

    # -- the reference's validation losses (csrc/losses.hip; INTEGRATION.md "Validation losses") --
    def validation_losses(self, output_or_items, anno_paths=None):
        """One frame: `output_or_items` is a dict of predict(..., gt_labels=) -> its `losses` (the five floats under the reference's key
        names; ValueError when the call carried no ground truth or losses= is off).  A dataset: `output_or_items` is an iterable of
        predict_stream's items and anno_paths one annotation file (or array) per item, read the way evaluate_stream reads it
        (load_annotation) and renumbered 1..n in ascending label order -> {"frames": [losses per item], "mean": {key: mean over the
        frames that have it}, "n": frames}.  Per-frame values: the reference's for a batch of that one frame."""
        if isinstance(output_or_items, dict):
            if "losses" not in output_or_items:
                raise ValueError("validation_losses: the output carries no losses (construct with losses= and pass gt_labels= to predict)")
            return dict(output_or_items["losses"])
        if self.refiner_predictor.losses is None:
            raise ValueError("validation_losses: construct the MaskRefiner with losses=")
        if anno_paths is None:
            raise ValueError("validation_losses: anno_paths is required with a list of items")
        frames = []
        for item, anno_path in zip(output_or_items, anno_paths):
            anno = load_annotation(anno_path, item[0], self.dataset, self._resize)
            if anno.ndim != 2:
                raise ValueError("annotation must be a single-channel label image")
            out = self.predict(item[0], item[1], item[2], mask_scores=item[4] if len(item) > 4 else None, gt_labels=compact_labels(anno))[1]
            frames.append(dict(out["losses"]))
        return {"frames": frames, "mean": mean_losses(frames), "n": len(frames)}

    # -- COCO AP of the initial and the refined masks (csrc/cocoap.hip; INTEGRATION.md "COCO AP of initial and refined masks") --
    def validation_ap(self, items, anno_paths, workers=2, batch=1, boundary=False, dilation_ratio=0.02):
        """The number the reference's COCOEvaluator prints after an evaluation period, for the refined masks and for the initial masks
        they came from.  items: predict_stream's; anno_paths: one annotation file (or array) per item, read with load_annotation and
        renumbered 1..n in ascending label order (compact_labels): one ground truth per label.  The initial masks are scored with the
        item's mask_scores (else 1.0), the refined ones with the predictor's instance scores, taken with their masks from the device
        tensors of the output dict.  -> {"initial": {"stats": f64 [12], "results": detectron2's dict}, "refined": {...}, "n": frames}.
        boundary=True: additionally "initial_boundary" and "refined_boundary" of the same shape, Boundary AP (CocoAP("boundary"), the
        reference's tools/evaluate_coco_boundary_ap.py) of the same masks with the dilation distance dilation_ratio x the frame's diagonal."""
        from collections import deque
        from .coco_ap import CocoAP
        dev = self.refiner_predictor.device
        aps = {"initial": CocoAP("segm", dev), "refined": CocoAP("segm", dev)}
        if boundary:
            aps.update({k + "_boundary": CocoAP("boundary", dev, dilation_ratio=dilation_ratio) for k in ("initial", "refined")})
        stages = [[ap for k, ap in aps.items() if k.startswith(s)] for s in ("initial", "refined")]
        seen = deque()                               # (initial masks, rgb path, mask scores) of the items predict_stream has pulled, in order

        def tee():
            for item in items:
                seen.append((item[2], item[0], item[4] if len(item) > 4 else None))
                yield item

        n = 0
        for res, anno_path in zip(self.predict_stream(tee(), workers=workers, batch=batch), anno_paths):
            init, rgb_path, init_scores = seen.popleft()
            anno = load_annotation(anno_path, rgb_path, self.dataset, self._resize)
            if anno.ndim != 2:
                raise ValueError("annotation must be a single-channel label image")
            gt = compact_labels(anno)
            init = np.asarray(init)
            init = (init != 0).reshape((-1,) + gt.shape)
            scores = np.ones(len(init), np.float32) if init_scores is None else check_scores(init_scores, len(init))
            for ap in stages[0]:
                ap.update(init, scores, gt)
            inst = res[1].get("instances")
            for ap in stages[1]:
                if inst is not None:
                    ap.update(inst.pred_masks, inst.scores, gt)
                else:
                    ap.update(np.zeros((0,) + gt.shape, np.uint8), np.zeros(0, np.float32), gt)
            n += 1
        return dict({k: {"stats": ap.summarize(), "results": ap.results()} for k, ap in aps.items()}, n=n)

    # -- the predicted error maps of one frame: scored against a ground truth, painted over the image (csrc/errhead.hip) --
    def _error_engine(self, h, w, n_masks=64):
        return self.refiner_predictor.model.engine_for(h, w, 1, n_masks)

    def _error_classes(self, eng, output, head):
        """The class map u8 [1,H,W] of `head`: the one decode_errors put into `output`, or decoded from the logits now."""
        if head + "_classes" in output:
            return output[head + "_classes"][None].contiguous()
        logits = output[head]
        return eng.error_decode(logits[None].contiguous(), (0, logits.shape[0]))[0]

    def score_error_maps(self, output, initial_masks, gt_masks):
        """How good is the error estimate of one frame: `output` is a dict of predict(); initial_masks / gt_masks are [N,H,W] /
        [Ng,H,W] arrays (non-zero = inside) at the network's frame size.  The explicit TP / TN / FP / FN maps
        (explicit_error_estimation/util.py:62-99) and the confusion table against the predicted classes
        (util.py:29-54, targets of model.py:185-227) are computed on the device.
        -> {head: {"confusion": int64 [C+1,C], "iou": [C], "iou_all", "iou_err", "accuracy"}} for every error head in `output`."""
        from . import error_maps as em
        et = self.refiner_predictor.cfg.MODEL.INS_EMBED_HEAD.ERROR_TYPE
        u8 = lambda m: np.ascontiguousarray((np.asarray(m) != 0).astype(np.uint8))[None]
        init, gt = u8(initial_masks), u8(gt_masks)
        h, w = init.shape[-2:]
        eng = self._error_engine(h, w, max(init.shape[1], gt.shape[1]))
        explicit = eng.error_maps(self._dev(init), self._dev(gt))
        res = {}
        for head, kind in (("eee_boundary", "boundary"), ("eee_mask", "region")):
            if head not in output:
                continue
            table = eng.error_score(self._error_classes(eng, output, head), explicit, kind, et)[0].cpu().numpy()
            res[head] = dict(em.iou_from_confusion(table), confusion=table, iou_err=em.iou_err(table, et))
        return res

    def visualize_errors(self, bgr, output, head="eee_boundary", palette=None):
        """The picture of eval/eval_utils.py:308-328: the predicted error classes of `head` painted over `bgr` (numpy u8 [H,W,3] at
        the network's frame size) -> numpy u8 [H,W,3].  palette: per class a (B, G, R) colour or None; default
        error_maps.DEFAULT_PALETTE of the configured ERROR_TYPE."""
        from . import error_maps as em
        if palette is None:
            palette = em.DEFAULT_PALETTE[self.refiner_predictor.cfg.MODEL.INS_EMBED_HEAD.ERROR_TYPE]
        bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
        eng = self._error_engine(bgr.shape[0], bgr.shape[1])
        return eng.error_overlay(self._dev(bgr[None]), self._error_classes(eng, output, head), palette)[0].cpu().numpy()

    def predict_stream(self, items, workers=2, batch=1):
        """items: iterable of (rgb_path, depth_path, initial_masks[, fg_mask[, mask_scores]]) -> yields predict()'s tuple per item, in
        order (mask_scores: required with nms=).
        The reference's evaluation loop (eval/eval_utils.py:235-286) calls predict() frame after frame; the host side of a frame -
        file decoding and, above all, the TELEA depth in-painting (9-14 ms, two to three times the refiner's GPU time) - is
        independent of the previous frame's refinement, so it runs ahead on `workers` threads (the in-painting is a ctypes call
        and releases the GIL; the workers' device work - resize, depth normalisation, and with batch > 1 the upload of the frame -
        goes to their own HIP stream).

        batch = k > 1: k consecutive frames of one size are refined by ONE engine call (the batched form of a1 ... a11 the
        reference lacks: it always runs batch 1, predictor.py:358), with the next batch already enqueued while the results of the
        current one are copied out - the GPU's batched throughput through the reference's own adapter API.  The per-frame tuples
        are the ones predict() returns (`seconds` = the batch's device time / k); a frame's logits may differ from its batch-1
        logits in the last bits (split-K partitions follow the launch size), which tests/test_gpu_network.py bounds and explains."""
        if self.refiner_predictor.zoom is not None:
            raise ValueError("zoom: predict_stream has no zoomed form; call predict() per frame (or construct without zoom=)")
        if self.refiner_predictor.seeding is not None:
            raise ValueError("seeding: predict_stream has no seeding form; call predict() per frame (or construct without seeding=)")
        if self.refiner_predictor.scene is not None:
            raise ValueError("scene: predict_stream has no scene form; call predict() per frame (or construct without scene=)")
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        import threading
        dev = self.refiner_predictor.device
        sides = {}
        k = max(1, int(batch))

        def load(item):
            tid = threading.get_ident()
            if tid not in sides:
                sides[tid] = torch.cuda.Stream(device=dev)
            side = sides[tid]
            with torch.cuda.stream(side):
                fr = self._load(item[0], item[1], item[2], item[4] if len(item) > 4 else None)
                if k > 1:                        # the frame goes to the device here, off the main thread
                    m = fr["masks"]
                    fr["d_rgb"] = torch.from_numpy(fr["rgb"]).to(dev, non_blocking=True)
                    if fr.get("depth_dev") is not None:
                        fr["d_depth"] = fr["depth_dev"]          # already there (normalised, resized, in-painted on the device)
                    else:
                        fr["d_depth"] = None if fr["depth"] is None else torch.from_numpy(np.ascontiguousarray(fr["depth"])).to(dev, non_blocking=True)
                    # (0-255 masks upload as they are; what is neither bool nor uint8 is cast, here alone)
                    fr["d_masks"] = torch.from_numpy(np.ascontiguousarray(mask_bytes(m, False).astype(np.uint8, copy=False))).to(dev, non_blocking=True)
                    if fr["scores"] is not None:
                        fr["d_scores"] = torch.from_numpy(fr["scores"]).to(dev, non_blocking=True)
                    fr["ready"] = torch.cuda.Event()
                    fr["ready"].record(side)
                    side.synchronize()           # (pageable sources: the copies are complete when this returns)
                return fr

        def enqueue(frs):
            model = self.refiner_predictor.model
            n = max(f["d_masks"].shape[0] for f in frs)
            H_, W_ = frs[0]["d_rgb"].shape[:2]
            for f in frs:
                torch.cuda.current_stream().wait_event(f["ready"])
            two = self.refiner_predictor.depth_on and self.refiner_predictor.rgb_on
            B_ = len(frs)
            own = [f["d_masks"].shape[0] for f in frs]      # each frame's own masks among the n rows of the batch
            # B-frame tensors; test-time augmentation: the frames go straight into the first halves of 2B-frame buffers (the flip fills the rest)
            d_rgb, d_depth, d_masks = model.batch_buffers(B_, H_, W_, n, two)
            d_masks[:B_].zero_()
            for b, f in enumerate(frs):
                if f["d_masks"].shape[0]:
                    d_masks[b, :f["d_masks"].shape[0]] = f["d_masks"]
            d_scores = None
            if model.nms is not None:                       # NaN: no such mask (the rows of a frame with fewer than n)
                d_scores = torch.full((B_, n), float("nan"), dtype=torch.float32, device=dev)
                for b, f in enumerate(frs):
                    if f["d_masks"].shape[0]:
                        d_scores[b, :f["d_masks"].shape[0]] = f["d_scores"]
            img = [f["d_rgb"] if self.refiner_predictor.rgb_on else f["d_depth"] for f in frs]   # depth-only: the image IS the depth map
            torch.stack(img, out=d_rgb[:B_])
            if two:
                torch.stack([f["d_depth"] for f in frs], out=d_depth[:B_])
            return model.enqueue_batch(d_rgb, d_depth, d_masks, slots=max(32, n + 12), capacity=k, halves=model.tta, n_masks=own,
                                       d_scores=d_scores)

        def collect(frs, hd):
            outs, ms, host = self.refiner_predictor.model.collect_batch(hd, host_masks=True)
            for fr, output, refined in zip(frs, outs, host):
                # `seconds` of a streamed frame = its share of the batch's device time (+ the post-filter, if any, inside _finish)
                yield self._finish(fr, output, refined, time.time() - ms * 1e-3 / len(frs))

        with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
            it = iter(items)
            ahead = deque()
            depth = max(workers, 2 * k if k > 1 else 0)
            for item in it:
                ahead.append(pool.submit(load, item))
                if len(ahead) > depth:
                    break

            def next_frame():
                fr = ahead.popleft().result()
                nxt = next(it, None)
                if nxt is not None:
                    ahead.append(pool.submit(load, nxt))
                return fr

            if k == 1:
                while ahead:
                    yield self._refine(next_frame())
                return
            pending = None                        # (frames, handle) of the batch in flight
            carry = None                          # a loaded frame that did not fit the current group (other size)
            while ahead or carry is not None:
                group = [carry] if carry is not None else []
                carry = None
                while len(group) < k and ahead:
                    fr = next_frame()
                    if group and fr["d_rgb"].shape != group[0]["d_rgb"].shape:
                        carry = fr
                        break
                    group.append(fr)
                hd = enqueue(group)
                if pending is not None:
                    yield from collect(*pending)
                pending = (group, hd)
            if pending is not None:
                yield from collect(*pending)

    def evaluate_stream(self, items, anno_paths, workers=2, batch=1, cap=64):
        """predict_stream plus the evaluation step of the reference's loop (eval/eval_utils.py:240-250, 281-286, 337-338): yields
        (refined_masks, output, seconds, fg_mask, initial_metrics, refined_metrics) per item, in order.  anno_paths: one annotation file
        (or array) per item.  Per group of up to max(batch, 1) frames of one size the initial and the refined label maps are painted and
        their 2k pairs evaluated by ONE multilabel_metrics_batch call (csrc/evalbatch.hip) on a stream of its own, while
        predict_stream already has the next group enqueued.  cap: most labels per map the batched call handles; a frame above it is
        answered by the per-frame function."""
        from .evaluation import multilabel_metrics_batch
        from collections import deque
        k = max(int(batch), 1)
        dev = self.refiner_predictor.device
        seen = deque()                               # (initial masks, rgb path) of the items predict_stream has pulled, in order

        def tee():
            for item in items:
                seen.append((item[2], item[0]))
                yield item

        side = torch.cuda.Stream(device=dev)

        def evaluate(group):
            shape = group[0][1].shape
            preds = np.stack([label_map_from_masks(init, shape) for _, _, init in group] +
                             [label_map_from_masks(res[0], shape) for res, _, _ in group])
            gts = np.stack([anno for _, anno, _ in group] * 2)
            with torch.cuda.stream(side):
                metrics = multilabel_metrics_batch(preds, gts, cap=cap, device=dev)
            n = len(group)
            for i, (res, _, _) in enumerate(group):
                yield tuple(res) + (metrics[i], metrics[n + i])

        group = []
        for res, anno_path in zip(self.predict_stream(tee(), workers=workers, batch=batch), anno_paths):
            init, rgb_path = seen.popleft()
            anno = load_annotation(anno_path, rgb_path, self.dataset, self._resize)
            if anno.ndim != 2:
                raise ValueError("annotation must be a single-channel label image")
            if group and anno.shape != group[0][1].shape:
                yield from evaluate(group)
                group = []
            group.append((res, anno, init))
            if len(group) >= k:                      # predict_stream has the next group enqueued by now
                yield from evaluate(group)
                group = []
        if group:
            yield from evaluate(group)


class MaskRefinerTTA(MaskRefiner):
    """``MaskRefinerTTA(config_file, weights_file=..., dataset=...)`` of eval/un_eval_utils.py:79-81: MaskRefiner with horizontal-flip
    test-time augmentation.  predict() and predict_stream(batch=k) work as on MaskRefiner; the engine runs 2k frames."""

    def __init__(self, config_file=None, weights_file=None, dataset="OSD", decode_errors=False, cleanup=None, **kw):
        super().__init__(config_file, weights_file=weights_file, dataset=dataset, tta=True, decode_errors=decode_errors, cleanup=cleanup, **kw)
