"""Drop-in for ``maskrefiner.predictor.MaskRefinerPredictor`` (reference maskrefiner/predictor.py:207-359)
running on the MI355X HIP path.

Same constructor and ``predict`` signatures, same return structure (a list with one dict holding
``sem_seg`` [1,H,W] logits, ``eee_boundary`` [4,H,W] logits, ``panoptic_seg`` (f32 [H,W] labels, None)
and, when any instance survives, ``instances`` with ``pred_masks`` bool [K,H,W], ``scores``,
``pred_boxes``, ``pred_classes`` - reference model.py:304-356).  Deliberate differences:
  * none of the reference constructor's side effects (dataset loader, output dir, hard-coded
    weights path: predictor.py:226-243);
  * the initial-mask encoding, network and grouping all run on the GPU; ``predict_batch`` exposes the
    batched form the reference lacks (it always runs batch 1, predictor.py:358);
  * ``tta=True``: horizontal-flip test-time augmentation, which the reference's driver asks for (eval/un_eval_utils.py:78-81)
    but never defines - every frame and its W-mirror run as one forward of 2B frames, the logits are merged on the device
    (flip back, x-offset negated, averaged: INTEGRATION.md) and post-processing runs on the merged maps.
  * ``decode_errors=True``: every dict also carries, per error head, the class map (``eee_boundary_classes`` u8 [H,W] = the argmax
    of the logits), its histogram and the class counts inside every initial mask, all computed on the device (csrc/errhead.hip;
    INTEGRATION.md "Predicted error maps").  Off by default: the dicts then have the reference's keys only.
  * ``iterations=k``: the refined masks are fed back as the initial masks of a further pass, k passes in all, without leaving the
    device (csrc/iterate.hip; INTEGRATION.md "Iterative refinement"); ``until_converged=True`` stops as soon as a pass reproduces its
    input; ``track_initial=True`` reports which refined instance came from which initial mask.  Defaults: one pass, today's keys.
  * ``cleanup=Cleanup(...)`` / ``"largest"`` / ``"holes"``: the connected-component clean-up the reference's competing refiners run on
    the host (largest component, small holes), on the device right after post-processing (csrc/cleanup.hip; INTEGRATION.md
    "Connected-component clean-up"); ``instances`` gains ``cc_components`` / ``cc_removed`` / ``cc_filled``.  Default: none, today's keys.
  * ``perturb=Perturb(iou_target, seed=...)``: the uploaded initial masks are degraded on the device by the reference's ``perturb_seg``
    (a random walk of erosions / dilations until the IoU with the uploaded mask falls below the target: csrc/perturb.hip; INTEGRATION.md
    "Perturbed initial masks") before anything reads them - the encoding, the mirror of ``tta``, the first pass of ``iterations=k``
    (never the fed-back masks), ``track_initial``, the per-mask histograms.  Every dict gains ``perturbed_masks`` (u8 [n,H,W], 0 / 255)
    and ``perturb_report`` (i64 [n,4]: rounds, |seg & g|, |seg | g|, |seg|).  uint8 masks are perturbed as their bytes stand (> 127 is
    the mask, non-zero the ground truth), bool masks count as 0 / 255.  Default: none, today's keys.
  * ``nms=MaskNMS(thresh=0.7, on_top="large")``: the caller's initial masks are scored, overlapping proposals (SAM, MSMFormer, UCN with
    zoom-in); the reference's ``nms`` + ``combine_masks_with_NMS`` makes them disjoint on the device (csrc/masknms.hip; INTEGRATION.md
    "Overlapping initial masks") before anything else reads them - ``perturb``, the encoding, the mirror of ``tta``, the first pass of
    ``iterations=k``, ``track_initial``, the per-mask histograms all see its output as THE initial masks.  The scores are required
    (``predict(..., mask_scores=)``, ``predict_batch(..., scores_list=)``, ``enqueue_batch(..., d_scores=)``).  Every dict gains
    ``nms_masks`` (u8 [count,H,W], 0 / 255, disjoint), ``nms_source`` (i64 [count]: the input index of each), ``nms_scores`` (f32 [count])
    and ``nms_report`` (i64 [2]: count, kept = survivors of the NMS before hidden ones drop out).  Default: none, today's keys.
  * ``cluster=MeanShift(num_seeds=100, kappa=20, iters=10, alpha=0.02, depth_threshold=None, seed=0)``: there are no initial masks yet,
    only the UCN base model's 64-channel pixel embeddings; its mean-shift clustering (``clustering_features``, ``filter_labels_depth``,
    eval/base_model.py:622-840 and :34-47) makes the initial masks on the device (csrc/meanshift.hip; INTEGRATION.md "Initial masks from
    pixel embeddings") and everything downstream - ``perturb``, the encoding, ``tta``, ``iterations``, ``track_initial`` - sees them as
    THE initial masks.  ``predict`` / ``predict_batch`` then take ``embeddings=`` (f32 [64,H,W] per frame) in place of masks and an
    optional ``depth_z=`` (f32 [H,W], required when ``depth_threshold`` is set).  Every dict gains ``cluster_masks`` (u8 [count,H,W], 0 /
    255, disjoint), ``cluster_ids`` (i32 [H,W]), ``cluster_seeds`` (f32 [num_seeds,64]: the climbed modes) and ``cluster_report`` (i64
    [4]: count, clusters before the depth filter, dropped by it, truncated).  Refused together with ``nms=``, with initial masks, and in
    ``enqueue_batch`` / ``predict_stream``.  Default: none, today's keys, nothing launched or allocated.
  * ``cluster=GaussianMeanShift(num_seeds=200, sigma=0.02, iters=10, epsilon=0.05, subsample=5, min_pixels=300, imp=IMP(9, True),
    seed=0)``: the same place for the third family of base model, UOIS-Net-3D, whose Depth Seeding Network gives a foreground map and a
    3-D centre vote per pixel: the Gaussian mean shift of ``DSNWrapper.cluster`` and the IMP of ``process_initial_masks``
    (uois/src/segmentation.py:129-187, :425-491) make the initial masks on the device (csrc/gms.hip; INTEGRATION.md "Initial masks from
    centre votes").  ``predict`` / ``predict_batch`` take ``center_votes=`` (f32 [3,H,W] per frame, xyz + offsets, finite) and ``fg=``
    (u8 / bool [H,W]) in place of masks.  The keys of ``MeanShift`` (``cluster_seeds`` is f32 [num_seeds,3], ``cluster_report`` i64 [6]:
    count, clusters found, dropped by ``min_pixels``, truncated, emptied by the IMP, fg pixels) and ``cluster_raw_ids`` (i32 [H,W]: the
    map before the IMP), ``cluster_centers`` (f32 [count,3]).  The same refusals; the input of the other clusterer is a ``ValueError``.
  * ``seeding=DepthSeeding(weights_or_path, negate_y=True)`` beside ``cluster=GaussianMeanShift.uois()``: the votes and the foreground
    come from UOIS-Net-3D's Depth Seeding Network on the device (csrc/dsn.hip, csrc/plan_dsn.hip, quber_amd/seeding; INTEGRATION.md
    "Initial masks from a depth image").  ``predict`` / ``predict_batch`` take ``xyz=`` (f32 [H,W,3] or [3,H,W] per frame: the organised
    point cloud, NaN where there is no depth; H and W multiples of 16) in place of ``center_votes=`` / ``fg=``; the network's votes and
    foreground go to the clustering as device pointers on the same stream, and the dicts are those of the same votes handed over from
    the host, bit for bit.  Only the three class counts per frame are read back: the seeded draw of a frame's first seed needs its
    foreground count.  Every dict gains ``seeding_fg`` (u8 [H,W]: 0 background, 1 table, 2 objects) and ``seeding_report`` (i64 [3]: the
    pixels of each class).  ``xyz=`` is a ``ValueError`` without ``seeding=``, together with ``center_votes=`` / ``fg=`` / masks, with a
    ``cluster=`` that is not a ``GaussianMeanShift``, and in ``enqueue_batch`` / ``predict_stream``.  ``camera=`` (a
    ``quber_amd.camera.Camera``) with ``depth_z=`` (f32 [H,W] per frame, metres) takes the place of ``xyz=``: the network's first kernel
    back-projects the depth image (INTEGRATION.md "From a depth image"), the dicts are those of ``xyz=xyz_np(depth_z, camera)``, and the
    same refusals apply, plus a missing or misshapen ``depth_z``.
  * ``region=RegionRefinement(weights_or_path, padding=0.25, threshold=0.5, crop=224, chunk=20)`` beside ``cluster=GaussianMeanShift()``:
    the third stage of UOIS-Net-3D, its Region Refinement Network (``rrn_preprocess``, ``RRNWrapper.run_on_batch``, ``rrn_postprocess``,
    uois/src/segmentation.py:294-423, :516-560) on the device (csrc/rrn.hip, csrc/plan_rrn.hip, quber_amd/region; INTEGRATION.md "Refined
    initial masks of the third family"), right after the clustering and before ``nms`` / ``scene`` / ``perturb`` / the encoding: every
    clustered mask is cropped with a padded box from the frame's bytes (standardised as the reference does), refined by the network in
    chunks of ``chunk`` crops, and painted back far objects first; the refined, compacted masks replace the clustered ones as THE initial
    masks.  z is plane 2 of ``xyz=`` under ``seeding=``; otherwise ``depth_z=`` (f32 [H,W] per frame) is required beside
    ``center_votes=`` / ``fg=``.  The per-frame cluster counts are read back once to build the crop list (the seeded path already reads
    three counts per frame).  Every dict gains ``region_masks`` (u8 [count,H,W], 0 / 255, disjoint), ``region_ids`` (i32 [H,W]),
    ``region_source`` (i64 [count]: the cluster id each refined mask came from), ``region_rois`` (i32 [clusters,4]) and ``region_report``
    (i64 [4]: refined masks, clusters that vanished, pixels painted, pixels painted over); the ``cluster_*`` entries keep the masks
    before the network.  ``RegionRefinement(final_close_morphology=True, ksize=9)`` opens and closes every refined id afterwards (the
    reference's pass of that name); ``region_report`` is then i64 [5], its last entry the ids the close removed.  A ``ValueError`` without a ``GaussianMeanShift``, without a z plane, and - as ``cluster=`` - in ``enqueue_batch``
    / ``predict_stream``.  Default: none - nothing imported, allocated or launched, today's keys.
  * ``zoom=ZoomIn(crop=224, padding=0.25, min_overlap=0.5)``: the second, zoomed-in pass of the reference's base models (``crop_rois`` /
    ``match_label_crop``, eval/base_model.py:843-961) without leaving the device (csrc/zoom.hip; INTEGRATION.md "Zoom-in refinement"):
    every instance of pass 1 - run with all configured options, through post-processing and ``cleanup`` - is cropped with a padded box,
    resized to crop x crop together with its own mask, refined by the same network as a batch of crops (same ``tta``, ``iterations``,
    ``cleanup``; no ``perturb``, ``nms``, ``decode_errors``, ``track_initial``), and the crop results that agree with the mask they came
    from are painted back, far objects first.  ``instances`` then holds the zoomed result (``pred_masks``, ``scores``, ``pred_boxes``,
    ``pred_classes`` all 0, ``zoom_source`` i64 [count,2]: first-pass id, crop-pass id); pass 1's move to ``coarse_instances``; the dict
    gains ``zoom_ids`` (i32 [H,W]), ``zoom_rois`` (i32 [k,4]) and ``zoom_report`` (i64 [4]: crops, kept, kept without a final id, count);
    ``sem_seg``, ``panoptic_seg`` and the error heads stay pass 1's.  ``predict`` and ``predict_batch``; ``enqueue_batch`` /
    ``predict_stream`` refuse it.  Default: none, today's keys, nothing launched or allocated.
  * ``losses=Losses(...)`` (``Losses.from_cfg(cfg)`` reads the reference's keys) together with a call's ``gt_labels=`` (``predict``,
    ``predict_batch``, ``enqueue_batch``: the ground-truth label map(s), integer, 0 = none, 1..n <= 254): the reference's training targets
    and the five values of its loss dict for every frame, on the device (csrc/losses.hip; INTEGRATION.md "Validation losses") - targets
    from the ground truth, explicit error maps from the initial masks the network actually saw (after ``nms`` / ``perturb``), losses of
    the pass's final logits (the merged ones under ``tta``).  Every dict gains ``losses`` ({loss_sem_seg, loss_center, loss_offset,
    loss_eee_*: float}, per frame), ``loss_terms`` (the raw sums) and, with ``keep_targets=True``, ``loss_targets``.  Refused together
    with ``iterations > 1`` or ``zoom=``.  Default, or a call without ``gt_labels``: nothing launched, today's keys.
  * ``scene=ScenePerturb(seed=0, max_masks=64, min_mask_ratio=0.01)``: the call's masks are the frame's GROUND TRUTH and its instance list
    is degraded on the device the way the reference builds its training inputs (tools/ours/perturbate_masks.py:101-205: false
    positives and over- / under-segmentations from ``proposals=`` (u8 / bool [P,H,W] per frame, may be absent), merge, split, delete:
    csrc/scene.hip; INTEGRATION.md "Scene-level perturbation") after ``nms`` and before ``perturb``; the mask rows of the pass are
    ``max_masks`` and everything downstream sees the scene's masks as THE initial masks.  Every dict gains ``scene_masks`` (u8
    [count,H,W], 0 / 255), ``scene_info`` (i64 [count,4]: kind, source, members, split) and ``scene_report`` (i64 [8]: count, n_fp, n_gs,
    ground truths kept, absorbed, splits, deleted, dropped).  ``predict`` and ``predict_batch``; refused together with ``cluster=`` or
    ``zoom=`` and in ``enqueue_batch`` / ``predict_stream``.  Default: none, today's keys, nothing launched or allocated.
There is no CPU fallback: construction fails if the HIP library or a GPU is missing.
"""
import os
import warnings
from dataclasses import dataclass

import numpy as np
import torch

from .. import arch, config as qconfig, engine as qengine
from ..cleanup import Cleanup
from ..masknms import MaskNMS, check_scores
from ..gms import IMP_LDS_BYTES, GaussianMeanShift, imp_plane_bytes
from ..meanshift import CHANNELS as CLUSTER_CHANNELS, MeanShift
from ..perturb import Perturb
from ..scene import MAX_SLOTS as SCENE_MAX_SLOTS, ScenePerturb
from ..structures import Boxes, Instances
from ..losses import Losses
from ..zoom import ZoomIn

LABEL_DIVISOR = 1000  # maskrefiner/data/datasets/register_uoais_sim_panoptic.py:177-186


def load_checkpoint(path):
    """detectron2 .pth ({'model': state_dict}) or a plain state_dict / .npz -> name -> numpy f32."""
    if path.endswith(".npz"):
        z = np.load(path)
        return {k: z[k] for k in z.files}
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd = ck.get("model", ck) if isinstance(ck, dict) else ck
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in sd.items()}


def same_segmentation(table):
    """table int [B,n+1,m+1] of Engine.overlap_ids (row / column 0 = no instance) -> bool [B]: the two label maps describe the same
    segmentation, i.e. every row and every column holds at most one non-zero cell and row 0 / column 0 none besides [0][0].  The next
    pass's encoding depends on the masks as sets only, so a frame for which this holds has reached a fixed point."""
    nz = table != 0
    ok = (nz.sum(2) <= 1).all(1) & (nz.sum(1) <= 1).all(1)
    return ok & ~nz[:, 0, 1:].any(1) & ~nz[:, 1:, 0].any(1)


def match_initial(table, area, n, k):
    """table int [N,K+1] / area int [K+1] of Engine.overlap_masks for one frame, its n initial masks and k instances ->
    (initial_overlap i64 [n,k+1], initial_index i64 [k], initial_iou f32 [k]): per instance the initial mask of the largest IoU
    (inter / (|mask| + area - inter) in float64, the first index wins ties; -1 / 0 when no initial mask touches it)."""
    tab = table[:n, :k + 1].to(torch.int64)
    if n == 0 or k == 0:
        return tab, torch.full((k,), -1, dtype=torch.int64, device=tab.device), torch.zeros((k,), dtype=torch.float32, device=tab.device)
    inter = tab[:, 1:].to(torch.float64)
    size = table[:n].sum(1, dtype=torch.int64).to(torch.float64)          # every pixel of a mask has some id: the row sum is |mask|
    union = size[:, None] + area[1:k + 1].to(torch.float64)[None] - inter
    iou = torch.where(union > 0, inter / union.clamp(min=1.0), torch.zeros_like(union))
    best = iou.max(0).values
    down = torch.arange(n, 0, -1, device=tab.device)[:, None]             # the first index among equals (argmax promises no order)
    first = n - ((iou == best[None]) * down).max(0).values
    touched = best > 0
    return tab, torch.where(touched, first, torch.full_like(first, -1)), torch.where(touched, best, torch.zeros_like(best)).to(torch.float32)


@dataclass(frozen=True)
class RefineOptions:
    """The options of the module docstring, validated and parsed once.  MaskRefiner, MaskRefinerPredictor and RefinerModel take them as
    keywords and hand this record on; each holds it as `options` and its fields as plain attributes (`model.tta`, `model.nms`, ...)."""
    tta: bool = False                 # every frame and its W-mirror in one forward of 2B frames, logits merged on the device
    decode_errors: bool = False       # per error head the class map, its histogram and the per-mask class counts in every dict
    iterations: int = 1               # passes per call, the refined masks fed back on the device
    until_converged: bool = False     # stop at a fixed point (predict / predict_batch; the stream always runs the fixed count)
    track_initial: bool = False       # initial_overlap / initial_index / initial_iou in every dict
    cleanup: Cleanup = None           # connected-component clean-up right after every post-processing pass
    perturb: Perturb = None           # the initial masks degraded on the device before anything reads them
    nms: MaskNMS = None               # scored, overlapping initial masks made disjoint on the device before anything else reads them
    zoom: ZoomIn = None               # a second pass on a padded, resized crop of every instance, pasted back on the device
    losses: Losses = None             # with a call's gt_labels=: the reference's training targets and loss dict of every frame, on the device
    cluster: object = None            # a MeanShift (pixel embeddings) or a GaussianMeanShift (centre votes): the initial masks are clustered on the device, before anything else
    scene: ScenePerturb = None        # the uploaded masks are a frame's ground truth: its instance list is degraded on the device (after nms, before perturb)

    @classmethod
    def parse(cls, tta=False, decode_errors=False, iterations=1, until_converged=False, track_initial=False, cleanup=None, perturb=None,
              nms=None, zoom=None, losses=None, cluster=None, scene=None):
        if int(iterations) < 1:
            raise ValueError("iterations must be >= 1")
        losses = Losses.parse(losses)
        if losses is not None and int(iterations) > 1:
            raise ValueError("losses: not with iterations > 1 (the last pass's input exists only as a label map: left out)")
        if losses is not None and zoom is not None:
            raise ValueError("losses: not with zoom= (the crop pass has no ground truth: left out)")
        if perturb is not None and not isinstance(perturb, Perturb):
            raise ValueError(f"perturb={perturb!r}: expected None or a quber_amd.perturb.Perturb")
        zoom, nms = ZoomIn.parse(zoom), MaskNMS.parse(nms)
        if not isinstance(cluster, GaussianMeanShift):       # either clusterer: UCN's embeddings (MeanShift) or UOIS-Net-3D's centre votes
            if cluster is not None and not isinstance(cluster, MeanShift):
                raise ValueError(f"cluster={cluster!r}: expected None, a quber_amd.meanshift.MeanShift or a quber_amd.gms.GaussianMeanShift")
            cluster = MeanShift.parse(cluster)
        if cluster is not None and nms is not None:
            raise ValueError("cluster: not with nms= (the clustering's masks are disjoint and have no scores)")
        scene = ScenePerturb.parse(scene)
        if scene is not None and cluster is not None:
            raise ValueError("scene: not with cluster= (the clustering's masks are no ground truth: left out)")
        if scene is not None and zoom is not None:
            raise ValueError("scene: not with zoom= (left out)")
        return cls(bool(tta), bool(decode_errors), int(iterations), bool(until_converged), bool(track_initial), Cleanup.parse(cleanup),
                   perturb, nms, zoom, losses, cluster, scene)

    def for_crops(self):
        """The crop pass of zoom: the same tta, iterations and cleanup; nothing that concerns the caller's initial masks."""
        return RefineOptions(tta=self.tta, iterations=self.iterations, cleanup=self.cleanup)


@dataclass(slots=True)
class PassResult:
    """What device_pass enqueued for B frames: the engine, the last pass's logits and post tables, the initial masks u8 [B,N,H,W] as
    the network saw them, and what refine() / track() / decode() / perturb_masks() / nms_masks() / scene_masks() returned (None: option off; own_nm: under scene, the NMS's own counts).  own: per
    frame, how many of the N mask rows are the frame's own - the rows of initial_overlap, perturbed_masks and nms_masks; a sequence
    indexed by frame (under nms in the stream: a pinned tensor the NMS's counts are copied into, valid once e1 has passed).
    enqueue_batch alone fills the rest - this record is its handle: the pre-extracted masks u8 [B,slots,H,W], the pinned instance
    counts and refine_converged_at, the events around the batch."""
    eng: object
    B: int
    logits: object
    post: dict
    d_masks: object = None
    own: object = None
    it: dict = None
    ov: tuple = None
    err: dict = None
    pt: tuple = None
    nm: dict = None
    cl: dict = None
    ls: dict = None
    sn: dict = None
    rg: dict = None        # what region_masks() returned (the Region Refinement Network stage), or None
    own_nm: object = None
    masks: object = None
    slots: int = 0
    count: object = None
    conv: object = None
    e0: object = None
    e1: object = None


def mask_bytes(m, as_bytes, binarise=False):
    """The bytes an array of initial masks uploads as.  uint8 goes as it stands; bool as 0 / 1 - the encoder tests for non-zero
    (csrc/encode.hip) - or, with as_bytes (perturb or nms will read the byte values: perturb_seg thresholds at 127), as 0 / 255.  The
    call sites differ in the rest, and each keeps its bytes: MaskRefiner._load passes as_bytes=True whatever the options (a bool mask is
    0 / 255 from there on) and leaves every other dtype to predict(), which sends it through predict_batch; predict_stream's load casts
    what is left to uint8; predict_batch alone passes binarise=True: every dtype goes through `m != 0`, so without as_bytes a uint8 255
    uploads as 1 there and as 255 through predict() - the same network input, different bytes."""
    m = np.asarray(m)
    if m.dtype == np.uint8 and (as_bytes or not binarise):
        return m
    if m.dtype != np.bool_:
        if not binarise:
            return m
        m = m != 0
    return m.view(np.uint8) * np.uint8(255) if as_bytes else m.view(np.uint8)


class _FrameStaging:
    """Buffers of the batch-1 call path for one frame size, allocated once: ONE pinned host block and ONE device block for the
    frame's inputs (bgr | depth | initial masks, uploaded in a few pipelined pieces), the device-side intermediates, and pinned
    word for the instance count.  frames = 2 (test-time augmentation): the device block holds every input for two frames - the
    uploaded frame in slot 0, its mirror in slot 1 (bgr [2,H,W,3] | depth [2,H,W,3] | masks [2,N,H,W]); the host block one."""

    def __init__(self, eng, n_cap, frames=1, iterate=False, track=False):
        H, W, dev = eng.H, eng.W, eng.device
        hw = H * W
        self.n_cap = n_cap
        self.frames = frames
        self.pin_in = torch.empty(6 * hw + n_cap * hw, dtype=torch.uint8).pin_memory()
        self.np_in = self.pin_in.numpy()
        self.dev_in = torch.empty(frames * (6 * hw + n_cap * hw), dtype=torch.uint8, device=dev)
        self.offsets = torch.empty((frames, 3, H, W), dtype=torch.float32, device=dev)
        self.post = eng.alloc_post(1)
        self.pin_count = torch.empty((2,), dtype=torch.int32).pin_memory()     # instance count, refine_converged_at
        self.done = torch.cuda.Event()
        self.iterate, self.track = iterate, track
        # iterations > 1: the two id maps (this pass's input, its refined map) and their overlap table; track_initial: the tables
        self.iter_bufs = _iter_buffers(eng, 1, frames, self.offsets) if iterate else None
        k1 = eng.cap + 1
        self.overlap = (torch.empty((1, n_cap, k1), dtype=torch.int32, device=dev),
                        torch.empty((1, k1), dtype=torch.int32, device=dev)) if track else None


def _iter_buffers(eng, B, frames, offsets=None):
    """(ids in, ids out, overlap table, offsets) of the passes >= 2 for B frames (frames = 2: and their mirrors)."""
    dev, k1 = eng.device, eng.cap + 1
    if offsets is None:
        offsets = torch.empty((frames * B, 3, eng.H, eng.W), dtype=torch.float32, device=dev)
    return (torch.empty((frames * B, eng.H, eng.W), dtype=torch.int32, device=dev),
            torch.empty((frames * B, eng.H, eng.W), dtype=torch.int32, device=dev),
            torch.empty((B, k1, k1), dtype=torch.int32, device=dev), offsets)


class RefinerModel:
    """The ``predictor.model`` object: ``model(list[dict]) -> list[dict]`` in the detectron2 convention
    (reference MaskRefiner.forward, model.py:115-358).  Engines are cached per (H, W, batch capacity)."""

    def __init__(self, cfg, state_dict, device, tta=False, decode_errors=False, iterations=1, until_converged=False,
                 track_initial=False, cleanup=None, perturb=None, nms=None, zoom=None, losses=None, cluster=None, scene=None, options=None):
        # options: a RefineOptions in place of the twelve keywords.  Its fields become plain attributes, which is what the code below
        # reads (a test and a tool switch model.decode_errors between calls)
        self.options = options or RefineOptions.parse(tta=tta, decode_errors=decode_errors, iterations=iterations, until_converged=until_converged,
                                                      track_initial=track_initial, cleanup=cleanup, perturb=perturb, nms=nms, zoom=zoom,
                                                      losses=losses, cluster=cluster, scene=scene)
        vars(self).update(vars(self.options))
        self._zoom_model = None   # the crop pass: a RefinerModel on the same cfg and weights, built by the first zoomed call
        self.debug_zoom = None    # tests: a list that receives, per zoomed call, the inputs and outputs of every stage
        self._perturb_dev = {}    # (frames, masks, H, W) -> the programs and targets of such a call on the device
        self._scene_dev = {}      # (frames, proposal rows, H, W) -> the draw tables of such a call on the device
        self.cfg = cfg
        self.state_dict = state_dict
        self.device = torch.device(device)
        self.top_k = 200 if cfg is None else int(cfg.MODEL.PANOPTIC_DEEPLAB.TOP_K_INSTANCE)
        assert 1 <= self.top_k <= 254, "the label-map encoding holds at most 254 instances per frame"
        self.debug_passes = None  # tests: a list that receives, per pass, its input ids, logits, post tables and refined ids
        self._engines = {}
        self._retired = {}        # (H, W) -> the engine a larger one replaced last; see engine_for
        self._staging = {}
        self.training = False

    def eval(self):
        return self

    def engine_for(self, h, w, batch, n_masks=64):
        key = (h, w)
        if self.iterations > 1:
            n_masks = max(n_masks, self.top_k)       # a pass >= 2 encodes a label map of up to top_k instances
        eng = self._engines.get(key)
        if eng is None or eng.qcfg.max_batch < batch or eng.qcfg.max_instances < n_masks:
            # grow, never shrink: alternating workloads must not trigger repeated multi-GB rebuilds
            if eng is not None:
                batch, n_masks = max(batch, eng.qcfg.max_batch), max(n_masks, eng.qcfg.max_instances)
                # not closed here: a batch enqueued on it may still be waiting for collect_batch (predict_stream keeps one batch in
                # flight).  The replaced engine is closed as soon as that batch has been collected (collect_batch), or - with nothing
                # in flight - right away; close() below takes whatever is left.
                if getattr(eng, "_in_flight", 0) > 0:
                    self._retired.setdefault(key, []).append(eng)
                else:
                    torch.cuda.current_stream().synchronize()      # its last launches may still be running
                    eng.close()
            qc = qengine.make_config(h, w, max_batch=max(batch, 1), max_instances=max(64, n_masks), cfg=self.cfg)
            eng = qengine.Engine(qc, self.device)
            eng.load_state_dict(self.state_dict)
            self._engines[key] = eng
            self._staging.pop(key, None)
        return eng

    def staging_for(self, eng, n_masks):
        key = (eng.H, eng.W)
        stg = self._staging.get(key)
        frames = 2 if self.tta else 1
        it, tr = self.iterations > 1, self.track_initial
        if stg is None or stg.n_cap < n_masks or stg.frames != frames or stg.iterate != it or stg.track != tr:
            stg = _FrameStaging(eng, max(64, n_masks), frames, it, tr)
            self._staging[key] = stg
        return stg

    def postprocess(self, eng, logits, out=None):
        """a8-a11 and, with `cleanup` set, the connected-component clean-up of their result (its report kept beside the tables)."""
        post = eng.postprocess(logits, out)
        if self.cleanup is not None:
            post["cc_report"] = eng.cleanup_post(logits, post, self.cleanup, post.get("cc_report"))
        return post

    def nms_masks(self, eng, d_masks, d_scores, B):
        """nms: the first B frames of d_masks u8 [>= B,N,H,W] (device) are replaced by the disjoint masks the mask NMS makes of them and
        their scores f32 [B,N] (a NaN score: no such mask - the padding of a frame with fewer masks), in place as far as the caller can
        tell (the kernels write a fresh tensor, which is copied back and kept for the output dicts).  -> what Engine.mask_nms returns,
        or None."""
        if self.nms is None:
            return None
        if d_scores is None:
            raise ValueError("nms: the masks' scores are required when nms= is set")
        if d_masks is None or d_masks.shape[1] == 0:
            return None
        src = d_masks[:B]
        nm = eng.mask_nms(src, d_scores, self.nms)
        src.copy_(nm["masks"])
        return nm

    def cluster_masks(self, eng, d_masks, cluster_in, B):
        """cluster: the first B frames of d_masks u8 [>= B,N,H,W] (device) are FILLED with the masks the mean-shift clustering makes of
        cluster_in = (embeddings f32 [B,64,H,W], first seeds i32 [B], depth_z f32 [B,H,W] or None), all on the device (the kernels write
        a fresh tensor, which is copied in and kept for the output dicts).  -> what Engine.meanshift returns, or None."""
        if self.cluster is None:
            return None
        if cluster_in is None:
            raise ValueError("cluster: this call path has no embeddings (predict and predict_batch take embeddings=)")
        if isinstance(self.cluster, GaussianMeanShift):      # cluster_in = (votes f32 [B,3,H,W], fg u8 [B,H,W], first i32 [B], draws i32 [B,S])
            from ..uois_chain import cluster_stage
            cl = cluster_stage(eng, self.cluster, cluster_in, d_masks.shape[1])
        else:
            emb, first, z = cluster_in
            cl = eng.meanshift(emb, first, self.cluster, d_masks.shape[1], z)
        d_masks[:B].copy_(cl["masks"])
        return cl

    def region_masks(self, eng, bgr, d_masks, cl, region_in, B):
        """region: the clustered masks of the first B frames are cropped, refined by the Region Refinement Network and painted back
        (RegionRefinement.refine), and d_masks[:B] are REPLACED by the refined, compacted masks - the pass's initial masks from here on.
        region_in = (the RegionRefinement, z f32 [B,H,W] on the device).  One small read-back, the per-frame cluster counts, builds the
        slot list.  -> what RegionRefinement.refine returns, or None."""
        if region_in is None:
            return None
        from ..uois_chain import region_stage
        region, z = region_in
        rg = region_stage(eng, region, bgr[:B], cl, d_masks.shape[1], z)
        d_masks[:B].copy_(rg["masks"])
        return rg

    def scene_masks(self, eng, d_masks, scene_in, nm, B):
        """scene: the first B frames of d_masks u8 [>= B,M,H,W] (device), M = scene.max_masks, are FILLED with the instance list the scene
        perturbation makes of scene_in = (ground truth u8 [B,N,H,W] - after nms when that is set -, n_gt i32 [B], proposals u8 [B,P,H,W],
        n_prop i32 [B]), all on the device; nm: what nms_masks returned for the ground truth (its count is then each frame's n_gt).
        -> what Engine.scene_perturb returns."""
        gt, n_gt, props, n_prop = scene_in
        if nm is not None:
            n_gt = nm["report"][:, 0].contiguous()
        P, key = props.shape[1], (B, props.shape[1], eng.H, eng.W)
        if key not in self._scene_dev:
            if len(self._scene_dev) >= 8:
                self._scene_dev.pop(next(iter(self._scene_dev)))
            d = self.scene.draws(B, P, eng.H, eng.W)
            self._scene_dev[key] = {k: torch.from_numpy(d[k].copy()).to(self.device) for k in
                                    ("fp_act", "gs_act", "merge_act", "split_act", "split_try", "delete_act")}
        sn = eng.scene_perturb(gt, props, n_gt, n_prop, self._scene_dev[key], self.scene.max_masks, self.scene.min_mask_ratio)
        d_masks[:B].copy_(sn["masks"])
        return sn

    def perturb_masks(self, eng, d_masks, B):
        """perturb: the first B frames of d_masks u8 [>= B,N,H,W] (device) are replaced by their perturbed versions, in place as far as
        the caller can tell (the kernel writes a fresh tensor, which is copied back and returned for the output dicts).
        -> (perturbed u8 [B,N,H,W], report i32 [B,N,4]) or None."""
        if self.perturb is None or d_masks is None or d_masks.shape[1] == 0:
            return None
        N, key = d_masks.shape[1], (B, d_masks.shape[1], eng.H, eng.W)
        if key not in self._perturb_dev:
            if len(self._perturb_dev) >= 8:
                self._perturb_dev.pop(next(iter(self._perturb_dev)))
            self._perturb_dev[key] = (torch.from_numpy(self.perturb.programs(B, N, eng.H, eng.W).copy()).to(self.device),
                                      torch.from_numpy(self.perturb.targets(B, N)).to(self.device))
        prog, tgt = self._perturb_dev[key]
        src = d_masks[:B]
        out, rep = eng.perturb_masks(src, prog, tgt)
        src.copy_(out)
        return out, rep

    # -- horizontal-flip test-time augmentation --
    def tta_alloc(self, B, H, W, n, depth=True, frames=2):
        """Empty 2B-frame device buffers (bgr, depth or None, masks [2B,n,H,W]): the caller fills frames [0, B) directly, the flip
        kernel fills [B, 2B)."""
        dev = self.device
        bgr = torch.empty((frames * B, H, W, 3), dtype=torch.uint8, device=dev)
        return bgr, torch.empty_like(bgr) if depth else None, torch.empty((frames * B, n, H, W), dtype=torch.uint8, device=dev)

    def batch_buffers(self, B, H, W, n, depth=True):
        """Empty device buffers a caller uploads B frames into, rows [0, B): B-frame tensors, or with tta the 2B-frame ones of tta_alloc
        (enqueue_batch: halves=True)."""
        return self.tta_alloc(B, H, W, n, depth, 2 if self.tta else 1)

    def initial_offsets(self, eng, masks, frames, out=None):
        """a1: the encoding of masks u8 [frames,N,H,W] -> f32 [frames,3,H,W] (`out`, if given); all zero for N = 0 or no masks."""
        if masks is not None and masks.shape[1]:
            return eng.encode(masks, out)
        if out is None:
            return torch.zeros((frames, 3, eng.H, eng.W), dtype=torch.float32, device=self.device)
        return out.zero_()

    def tta_logits(self, eng, bgr2, depth2, masks2, offsets=None, ready=False):
        """The augmented forward on 2B-frame buffers whose first halves hold the frames, all on the current stream: mirror the
        inputs into the second halves, a1 on all 2B frames (the mirrored frames' own encoding), one forward of 2B frames, merge
        -> logits f32 [B,planes,H,W] of the B frames.  `offsets`: an optional [2B,3,H,W] buffer for a1.  ready=True (a pass >= 2 of
        the iterative refinement): the images are mirrored already and `offsets` holds a1 of all 2B frames."""
        if not ready:
            eng.tta_flip_inputs(bgr2, depth2, masks2 if masks2 is not None and masks2.shape[1] else None)
            offsets = self.initial_offsets(eng, masks2, bgr2.shape[0], offsets)
        return eng.tta_merge(eng.forward(bgr2, depth2, offsets))

    def decode(self, eng, logits, d_masks=None):
        """decode_errors: enqueue, per enabled error head, the class map and histogram of `logits` [B,planes,H,W] and - given the
        initial masks u8 [B,N,H,W] on the device - the per-mask class counts.  -> {head: (classes, hist, mask_hist | None)} or None."""
        if not self.decode_errors:
            return None
        err = {}
        for head, (_, ncls) in eng.error_heads().items():
            cls, hist = eng.error_decode(logits, head)
            mh = None
            if d_masks is not None:
                mh = eng.error_mask_hist(cls, d_masks, ncls)
            err[head] = (cls, hist, mh)
        return err

    # -- iterative refinement (INTEGRATION.md "Iterative refinement") --
    def refine(self, eng, bgr, depth, logits, post, B, may_stop=False, bufs=None):
        """Passes 2 .. iterations on frames whose pass 1 has just been enqueued: relabel_panoptic(post) -> encode_label_map -> forward
        -> postprocess (into the same `post` tables), all on the current stream, nothing copied to the host unless may_stop and
        until_converged (the flags are then read after every pass).  bgr / depth: the buffers pass 1 ran on (test-time augmentation:
        2B frames, mirrors filled).  -> (logits, post, it) of the last pass; it: None for iterations == 1, else the passes run, the
        per-frame refine_converged_at (device, i32 [B]) and the last pass's refined map as compact ids."""
        if self.iterations == 1:
            return logits, post, None
        K = eng.cap
        ids_in, ids_out, table, offsets = bufs if bufs is not None else _iter_buffers(eng, B, 2 if self.tta else 1)
        conv = torch.zeros((B,), dtype=torch.int32, device=self.device)
        dbg = self.debug_passes
        snap = lambda d: {k: v.clone() for k, v in d.items()}
        eng.relabel_panoptic(post, mirror=self.tta, out=ids_in)
        if dbg is not None:
            dbg.append({"ids_in": None, "logits": logits, "post": snap(post), "ids_out": ids_in[:B].clone()})
        passes = 1
        for p in range(2, self.iterations + 1):
            eng.encode_label_map(ids_in, K, offsets)
            logits = self.tta_logits(eng, bgr, depth, None, offsets, ready=True) if self.tta else eng.forward(bgr, depth, offsets)
            self.postprocess(eng, logits, post)
            eng.relabel_panoptic(post, mirror=self.tta, out=ids_out)
            eng.overlap_ids(ids_in[:B], ids_out[:B], K, K, out=table)
            conv = torch.where((conv == 0) & same_segmentation(table), torch.full_like(conv, p), conv)
            passes = p
            if dbg is not None:
                dbg.append({"ids_in": ids_in[:B].clone(), "logits": logits, "post": snap(post), "ids_out": ids_out[:B].clone()})
            ids_in, ids_out = ids_out, ids_in
            if may_stop and self.until_converged and p < self.iterations and bool((conv > 0).all()):
                break
        return logits, post, {"passes": passes, "conv": conv, "ids": ids_in[:B]}

    def track(self, eng, d_masks, post, it, out=None):
        """track_initial: enqueue the overlap of the initial masks u8 [B,N,H,W] with the last pass's refined map -> (table, area) or None."""
        if not self.track_initial:
            return None
        ids = it["ids"] if it is not None else eng.relabel_panoptic(post)
        return eng.overlap_masks(d_masks, ids, eng.cap, out=out)

    # -- the one sequence predict_one, enqueue_batch and predict_batch run; they differ in who owns the buffers and where the host reads --
    # -- validation losses (INTEGRATION.md "Validation losses") --
    def upload_gt(self, gt_labels, B, H, W):
        """A call's gt_labels= -> None (losses off, or no ground truth with this call) or (labels i32 [B,H,W], the ids' masks u8
        [B,max(n_gt, 1),H,W], n_gt) on the device.  gt_labels: an integer label map [H,W] / [B,H,W] or a list of B maps, at the network's
        frame size, 0 = none, 1..n (n <= 254)."""
        if self.losses is None or gt_labels is None:
            return None
        lab = np.stack([np.asarray(g) for g in gt_labels]) if isinstance(gt_labels, (list, tuple)) else np.asarray(gt_labels)
        if lab.ndim == 2:
            lab = lab[None]
        if lab.shape != (B, H, W) or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError(f"gt_labels: expected {B} integer label map(s) of {(H, W)}, got {lab.dtype} {lab.shape}")
        n_gt = int(lab.max()) if lab.size else 0
        if int(lab.min()) < 0 or n_gt > 254:
            raise ValueError("gt_labels: ids outside 0..254")
        lab = np.ascontiguousarray(lab, dtype=np.int32)
        gt_masks = (lab[:, None] == np.arange(1, max(n_gt, 1) + 1, dtype=np.int32)[None, :, None, None]).view(np.uint8)
        return torch.from_numpy(lab).to(self.device), torch.from_numpy(gt_masks).to(self.device), n_gt

    def loss_stage(self, eng, logits, d_masks, gt, B):
        """losses: enqueue the targets of the ground-truth ids, the explicit error maps of the initial masks AS THE NETWORK SAW THEM (after
        nms / perturb) against the ground truth's masks, and the loss record of `logits` (the merged ones under tta).  gt: upload_gt()'s
        triple.  -> {"rec": f64 [B,LOSS_WORDS], "targets": Engine.loss_targets()'s dict, "heads", "explicit"} or None."""
        if self.losses is None or gt is None:
            return None
        labels, gt_masks, n_gt = gt
        tg = eng.loss_targets(labels, n_gt, self.losses)
        heads = eng.loss_heads(self.losses)
        explicit = None
        if heads:
            init = d_masks if d_masks.shape[1] else torch.zeros((B, 1, eng.H, eng.W), dtype=torch.uint8, device=self.device)
            explicit = eng.error_maps(init, gt_masks)
        return {"rec": eng.losses(logits, tg["targets"], explicit, self.losses, heads=heads), "targets": tg, "heads": heads, "explicit": explicit}

    def device_pass(self, eng, bgr, depth, masks, scores, B, *, may_stop, bufs=None, own=None, slots=None, gt=None, cluster_in=None, scene_in=None,
                    region_in=None):
        """Enqueues cluster (cluster_in: see cluster_masks) -> region (region_in: see region_masks) -> nms -> scene (scene_in: see scene_masks; nms then runs on ITS ground truth) -> perturb -> encode (tta: mirror, encode) -> forward -> postprocess ->
        refine -> track -> decode for B frames on the current stream -> PassResult.  bgr / depth (or None) u8 [f*B,H,W,3] and masks u8 [f*B,N,H,W] on the device, f = 2 under tta
        with the frames in the first halves; scores f32 [B,N] (required with nms).  Nothing is read back unless may_stop and
        until_converged (refine()).  bufs: predict_one's _FrameStaging - its offsets, post tables, iteration buffers and overlap tables
        are written instead of fresh tensors.  own: see PassResult; default all N rows.  slots (the stream): the first `slots` masks
        of every frame are extracted between track and decode, where the stream has always launched that."""
        N = masks.shape[1]
        cl = self.cluster_masks(eng, masks, cluster_in, B)
        rg = self.region_masks(eng, bgr, masks, cl, region_in, B)
        sn = None
        if self.scene is not None:
            if scene_in is None:
                raise ValueError("scene: this call path has no scene form (predict and predict_batch have)")
            nm = self.nms_masks(eng, scene_in[0], scores, B)
            sn = self.scene_masks(eng, masks, scene_in, nm, B)
        else:
            nm = self.nms_masks(eng, masks, scores, B)
        pt = self.perturb_masks(eng, masks, B)            # before the mirror, the encoding and everything else that reads the masks
        offsets = bufs.offsets if bufs is not None else None
        if self.tta:                                      # (either way the logits are a fresh tensor, owned by the caller through the dict)
            logits = self.tta_logits(eng, bgr, depth, masks, offsets)
        else:
            logits = eng.forward(bgr, depth, self.initial_offsets(eng, masks, B, offsets))
        post = self.postprocess(eng, logits, bufs.post if bufs is not None else None)
        logits, post, it = self.refine(eng, bgr, depth, logits, post, B, may_stop, bufs.iter_bufs if bufs is not None else None)
        d_masks = masks[:B]
        ov = self.track(eng, d_masks, post, it, (bufs.overlap[0][:, :N], bufs.overlap[1]) if bufs is not None and self.track_initial else None)
        rec = PassResult(eng, B, logits, post, d_masks=d_masks, own=[N] * B if own is None else own, it=it, ov=ov, pt=pt, nm=nm, cl=cl, sn=sn, rg=rg)
        if slots is not None:
            rec.slots = min(max(1, slots), eng.cap)
            rec.masks = eng.extract_masks(post, rec.slots)
        rec.err = self.decode(eng, logits, d_masks if it is None else None)    # (a pass >= 2 has no initial masks to attribute to)
        rec.ls = self.loss_stage(eng, logits, d_masks, gt, B)
        return rec

    # -- zoom-in refinement (INTEGRATION.md "Zoom-in refinement") --
    def zoom_model(self):
        """The crop pass: this model's cfg and weights with RefineOptions.for_crops()."""
        if self._zoom_model is None:
            self._zoom_model = RefinerModel(self.cfg, self.state_dict, self.device, options=self.options.for_crops())
        return self._zoom_model

    def zoom_pass(self, rec, bgr, depth, count, outs):
        """zoom: pass 2 on the instances pass 1 left in rec.post (bgr / depth: the B frames on the device; count: their instance counts
        on the host).  rois -> crops -> the crop pass in chunks of zoom.batch crops through enqueue_batch / collect_batch on the engine
        for (crop, crop) -> paste; then the dicts `outs` are rewritten: instances -> coarse_instances, the zoomed instances, zoom_ids /
        zoom_rois / zoom_report."""
        z, dev, eng, post, it = self.zoom, self.device, rec.eng, rec.post, rec.it
        B, S, n_ids = len(outs), self.zoom.crop, eng.cap
        ids = it["ids"] if it is not None else eng.relabel_panoptic(post)
        rois = eng.zoom_rois(ids, n_ids, z.padding)
        slots_h = np.array([(b, j) for b in range(B) for j in range(1, int(count[b]) + 1)], np.int32).reshape(-1, 2)
        T = len(slots_h)
        slots = torch.from_numpy(slots_h).to(dev)
        bgr, depth = bgr[:B], None if depth is None else depth[:B]
        C = eng.cap
        if T:
            bc, dc, mc = eng.zoom_crop(bgr, depth, ids, slots, rois, S)
            inner = self.zoom_model()
            parts, crop_count = [], []
            for a in range(0, T, z.batch):
                e = min(T, a + z.batch)
                hd = inner.enqueue_batch(bc[a:e], None if dc is None else dc[a:e], mc[a:e], slots=1, capacity=z.batch)
                ceng = hd.eng
                cid = hd.it["ids"] if hd.it is not None else ceng.relabel_panoptic(hd.post)
                table, area = ceng.overlap_masks(mc[a:e], cid, ceng.cap)
                parts.append((cid, hd.post["scores"], table.view(e - a, ceng.cap + 1), area))
                inner.collect_batch(hd)
                crop_count.extend(int(c) for c in hd.count.numpy())
            C = ceng.cap
            crop_ids, crop_scores, table, area = (torch.cat([p[i] for p in parts]).contiguous() for i in range(4))
            per_frame = np.bincount(slots_h[:, 0], weights=np.asarray(crop_count, np.float64), minlength=B)
            max_inst = int(min(254, max(1, per_frame.max())))          # an upper bound of every frame's final count
        else:
            e8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)
            bc, dc, mc = e8(0, S, S, 3), None if depth is None else e8(0, S, S, 3), e8(0, 1, S, S)
            crop_ids = torch.empty((0, S, S), dtype=torch.int32, device=dev)
            crop_scores = torch.empty((0, C), dtype=torch.float32, device=dev)
            table = area = torch.empty((0, C + 1), dtype=torch.int32, device=dev)
            max_inst = 1
        final = eng.zoom_paste(crop_ids, crop_scores, table, area, dc, slots, rois, B, z.min_overlap, max_inst)
        report = final["report"].cpu().numpy()
        if self.debug_zoom is not None:
            self.debug_zoom.append({"ids": ids.clone(), "bgr": bgr, "depth": depth, "slots": slots, "rois": rois, "bgr_crop": bc, "depth_crop": dc,
                                    "mask_crop": mc, "crop_ids": crop_ids, "crop_scores": crop_scores, "table": table, "area": area,
                                    "final": final})
        for b, r in enumerate(outs):
            k = int(report[b, 3])
            if "instances" in r:
                r["coarse_instances"] = r.pop("instances")
            r["zoom_ids"], r["zoom_rois"] = final["ids"][b], rois[b, :int(count[b])]
            r["zoom_report"] = torch.from_numpy(report[b].astype(np.int64))
            if k > 0:
                inst = Instances((eng.H, eng.W))
                inst.pred_masks = final["masks"][b, :k] != 0
                inst.scores = final["scores"][b, :k]
                inst.pred_boxes = Boxes(final["boxes"][b, :k])
                inst.pred_classes = torch.zeros((k,), dtype=torch.int64, device=dev)
                inst.zoom_source = final["source"][b, :k].to(torch.int64)
                r["instances"] = inst
        return outs

    def frame_dict(self, rec, b, k, masks_b, conv):
        """The reference's output dict of frame b (model.py:304-356) from a PassResult.  k: its instance count and masks_b: its k masks
        (bool, or None), conv: its refine_converged_at - all three read back by the caller.  The per-mask histograms keep all N rows
        here (results() trims them to the frame's own)."""
        eng, post, it, ov, pt, nm = rec.eng, rec.post, rec.it, rec.ov, rec.pt, rec.nm
        qc, logits_b = eng.qcfg, rec.logits[b]
        ncls, o = qc.error_classes, 4
        n = int(rec.own[b]) if rec.own is not None else None
        r = {"sem_seg": logits_b[0:1], "panoptic_seg": (post["panoptic"][b], None)}
        if qc.eee_boundary_on:                       # model.py:310-313
            r["eee_boundary"] = logits_b[o:o + ncls]
            o += ncls
        if qc.eee_mask_on:
            r["eee_mask"] = logits_b[o:o + ncls]
        for head, (cls, hist, mh) in (rec.err or {}).items():
            r[head + "_classes"], r[head + "_hist"] = cls[b], hist[b]
            if mh is not None:
                r[head + "_mask_hist"] = mh[b]
        if nm is not None:
            nn = n if rec.own_nm is None else int(rec.own_nm[b])
            r["nms_masks"], r["nms_source"], r["nms_scores"] = nm["masks"][b, :nn], nm["source"][b, :nn].to(torch.int64), nm["scores"][b, :nn]
            r["nms_report"] = nm["report"][b, :2].to(torch.int64)
        if rec.cl is not None:
            cl = rec.cl
            r["cluster_masks"], r["cluster_ids"], r["cluster_seeds"] = cl["masks"][b, :n], cl["ids"][b], cl["seeds"][b]
            r["cluster_report"] = cl["report"][b].to(torch.int64)
            if "raw_ids" in cl:                              # a GaussianMeanShift: the map before the IMP, and the clusters' centres
                r["cluster_raw_ids"], r["cluster_centers"] = cl["raw_ids"][b], cl["centers"][b, :n]
        if rec.rg is not None:                               # the cluster_* entries above keep the masks before the network
            rg, kc = rec.rg, int(rec.rg["counts"][b])
            if "report_host" not in rg:                      # read here, with the pass's other results: nothing waits for it inside the pass
                rg["report_host"] = rg["report"].cpu().numpy()
            kr = int(min(rg["report_host"][b, 0], n))
            r["region_masks"], r["region_ids"], r["region_source"] = rg["masks"][b, :kr], rg["ids"][b], rg["source"][b, :kr].to(torch.int64)
            r["region_rois"], r["region_report"] = rg["rois"][b, :kc], torch.from_numpy(rg["report_host"][b].astype(np.int64))
        if rec.sn is not None:
            r["scene_masks"], r["scene_info"] = rec.sn["masks"][b, :n], rec.sn["info"][b, :n].to(torch.int64)
            r["scene_report"] = rec.sn["report"][b].to(torch.int64)
        if pt is not None:
            r["perturbed_masks"], r["perturb_report"] = pt[0][b, :n], pt[1][b, :n].to(torch.int64)
        if it is not None:
            r["refine_passes"], r["refine_converged_at"] = it["passes"], int(conv)
        if ov is not None:
            r["initial_overlap"], first, iou = match_initial(ov[0][b], ov[1][b], n, k)
        if rec.ls is not None:                       # "host": the loss records f64 [B,LOSS_WORDS], read back by the caller
            r["losses"], r["loss_terms"] = self.losses.unpack(rec.ls["host"][b], rec.ls["heads"])
            if self.losses.keep_targets:
                r["loss_targets"] = {key: t[b] for key, t in rec.ls["targets"].items()}
        if k > 0:
            labels = post["labels"][b, :k]
            inst = Instances((eng.H, eng.W))
            inst.pred_masks = masks_b
            inst.scores = post["scores"][b, :k]
            inst.pred_boxes = Boxes(post["boxes"][b, :k])
            inst.pred_classes = (torch.div(labels, LABEL_DIVISOR, rounding_mode="floor") - 1).to(torch.int64)
            if ov is not None:
                inst.initial_index, inst.initial_iou = first, iou
            if "cc_report" in post:                  # row 1 + j of the frame's report: its j-th instance
                cc = post["cc_report"][b, 1:k + 1].to(torch.int64)
                inst.cc_components, inst.cc_removed, inst.cc_filled = cc[:, 0], cc[:, 1], cc[:, 2]
            r["instances"] = inst
        return r

    def results(self, rec, images=None):
        """The dicts of a PassResult: one D2H of the small per-frame tables, then mask extraction for exactly max(count) slots.  Under
        nms each frame's own initial masks are the `count` of the NMS's report, read here.  The per-mask histograms are trimmed to the
        frame's own rows (the stream keeps all N).  images (required with zoom=): the (bgr, depth) device tensors pass 1 ran on."""
        eng, post, B = rec.eng, rec.post, rec.B
        if rec.nm is not None:
            rec.own = [int(c) for c in rec.nm["report"][:, 0].cpu().numpy()]
        if rec.cl is not None:
            rec.own = [int(c) for c in rec.cl["report"][:, 0].cpu().numpy()]
        if rec.sn is not None:                       # the scene's list is what the network saw; the NMS's counts keep their own rows
            rec.own_nm = rec.own if rec.nm is not None else None
            rec.own = [int(c) for c in rec.sn["report"][:, 0].cpu().numpy()]
        count = post["count"].cpu().numpy()
        conv = rec.it["conv"].cpu().numpy() if rec.it is not None else np.zeros((B,), np.int32)
        if rec.ls is not None:
            rec.ls["host"] = rec.ls["rec"].cpu().numpy()
        kmax = int(count.max()) if B else 0
        masks = eng.extract_masks(post, kmax) if kmax > 0 else None
        outs = [self.frame_dict(rec, b, int(count[b]), masks[b, :int(count[b])].bool() if count[b] > 0 else None, conv[b]) for b in range(B)]
        for b, r in enumerate(outs):
            for key in r:
                if key.endswith("_mask_hist"):
                    r[key] = r[key][:rec.own[b]]
        if self.zoom is not None:
            if images is None:
                raise ValueError("zoom: this call path has no zoomed form (predict and predict_batch have)")
            outs = self.zoom_pass(rec, images[0], images[1], count, outs)
        return outs

    def predict_one(self, bgr, depth, masks, gt_labels=None):
        """The reference's call path (one frame per call, predictor.py:287-359) with nothing allocated per call but the
        outputs: the inputs go through one pinned block in a few pipelined H2D copies; the instance count comes back through
        a pinned word and exactly `count` masks are extracted."""
        if self.zoom is not None:
            raise ValueError("zoom: predict_one has no zoomed form; MaskRefinerPredictor.predict takes the batched path")
        if self.cluster is not None:
            raise ValueError("cluster: predict_one has no clustering form; MaskRefinerPredictor.predict takes the batched path")
        if self.scene is not None:
            raise ValueError("scene: predict_one has no scene form; MaskRefinerPredictor.predict takes the batched path")
        H, W = bgr.shape[:2]
        n = int(masks.shape[0])
        f = 2 if self.tta else 1                     # frames on the device: the frame [and its mirror]
        gt = self.upload_gt(gt_labels, 1, H, W)
        eng = self.engine_for(H, W, f, max(n, gt[2]) if gt is not None else n)
        stg = self.staging_for(eng, n)
        hw = H * W
        two = depth is not None
        stg.done.synchronize()                       # the previous call's H2D copies have read the pinned block
        # host copy into the pinned block and H2D, pipelined: the images first, then the masks in a few pieces - the DMA of a
        # piece runs while the host copies the next one (8 MB at N = 20: 0.3 ms of memcpy + 0.3 ms of PCIe, overlapped)
        o = (6 if two else 3) * hw
        od, om = 3 * f * hw, (6 if two else 3) * f * hw          # device offsets of depth and masks (f = 1: the host layout)
        np.copyto(stg.np_in[:3 * hw].reshape(H, W, 3), bgr, casting="unsafe")
        if two:
            np.copyto(stg.np_in[3 * hw:6 * hw].reshape(H, W, 3), depth, casting="unsafe")
        if f == 1:
            stg.dev_in[:o].copy_(stg.pin_in[:o], non_blocking=True)
        else:
            stg.dev_in[:3 * hw].copy_(stg.pin_in[:3 * hw], non_blocking=True)
            if two:
                stg.dev_in[od:od + 3 * hw].copy_(stg.pin_in[3 * hw:6 * hw], non_blocking=True)
        if n:
            # the encoder tests the mask bytes for non-zero (csrc/encode.hip), so uint8 / bool masks upload as they are (mask_bytes)
            step = max(1, (n + 2) // 3)
            for a in range(0, n, step):
                b = min(n, a + step)
                np.copyto(stg.np_in[o + a * hw:o + b * hw].reshape(b - a, H, W), masks[a:b], casting="unsafe")
                stg.dev_in[om + a * hw:om + b * hw].copy_(stg.pin_in[o + a * hw:o + b * hw], non_blocking=True)
        stg.done.record()
        d_bgr = stg.dev_in[:3 * f * hw].view(f, H, W, 3)
        d_dep = stg.dev_in[od:od + 3 * f * hw].view(f, H, W, 3) if two else None
        d_masks = stg.dev_in[om:om + f * n * hw].view(f, n, H, W)
        rec = self.device_pass(eng, d_bgr, d_dep, d_masks, None, 1, may_stop=True, bufs=stg, gt=gt)
        post = rec.post
        stg.pin_count[:1].copy_(post["count"], non_blocking=True)
        if rec.it is not None:
            stg.pin_count[1:].copy_(rec.it["conv"], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        if rec.ls is not None:
            rec.ls["host"] = rec.ls["rec"].cpu().numpy()
        k = int(stg.pin_count[0])
        # the dict owns clones: the staging's tables are the next call's
        rec.post = {key: post[key].clone() for key in ("panoptic", "labels", "scores", "boxes", "cc_report") if key in post}
        masks_b = None
        if k > 0:
            masks_b = eng.extract_masks(post, k)[0].view(torch.bool)      # the kernel writes 0 / 1 bytes
        # (the caller's ``.to('cpu')`` of the masks is a plain D2H copy into fresh pageable memory: 0.17 ms for 5 MB, which a
        # prefetch into a pinned buffer plus the copy out of it does not beat - tools/predict_profile.py)
        return self.frame_dict(rec, 0, k, masks_b, int(stg.pin_count[1]) if rec.it is not None else 0)

    # -- batched form on device-resident frames, split into "enqueue" and "collect" so that a caller can keep one batch in flight --
    def enqueue_batch(self, d_bgr, d_depth, d_masks, slots=32, capacity=0, halves=False, n_masks=None, d_scores=None, gt_labels=None, xyz=None,
                      camera=None):
        """d_bgr / d_depth: u8 [B,H,W,3] (depth None for single-stream configs), d_masks: u8 [B,N,H,W] on the device.  Enqueues a1 ...
        a11 and the extraction of the first `slots` instance masks of every frame on the current stream WITHOUT synchronising;
        returns a handle for collect_batch().  halves=True (test-time augmentation only): the tensors are 2B-frame buffers
        (tta_alloc) whose first halves hold the B frames.  n_masks: how many of the N masks are each frame's own (the rows of
        `initial_overlap` under track_initial; default: all N).  d_scores (required with nms=): f32 [B,N] on the device, the masks'
        scores, NaN for a mask that is not there; each frame's own masks are then the NMS's `count` and n_masks is not used.  gt_labels
        (with losses=): the B frames' ground-truth label maps on the host (upload_gt); every dict then carries `losses`."""
        if self.nms is not None and d_scores is None:
            raise ValueError("nms: d_scores is required when nms= is set")
        if self.zoom is not None:
            raise ValueError("zoom: enqueue_batch / predict_stream have no zoomed form; use predict or predict_batch")
        if xyz is not None:
            raise ValueError("xyz: enqueue_batch / predict_stream have no seeding form; use predict or predict_batch")
        if camera is not None:
            raise ValueError("camera: enqueue_batch / predict_stream have no seeding form; use predict or predict_batch")
        if self.cluster is not None:
            raise ValueError("cluster: enqueue_batch / predict_stream have no clustering form; use predict or predict_batch")
        if self.scene is not None:
            raise ValueError("scene: enqueue_batch / predict_stream have no scene form; use predict or predict_batch")
        if halves:
            assert self.tta and d_bgr.shape[0] % 2 == 0
        B, H, W = d_bgr.shape[:3]
        B = B // 2 if halves else B
        f = 2 if self.tta else 1                     # test-time augmentation: the engine runs the B frames and their mirrors
        gt = self.upload_gt(gt_labels, B, H, W)
        eng = self.engine_for(H, W, f * max(B, capacity), max(d_masks.shape[1], gt[2]) if gt is not None else d_masks.shape[1])      # (`capacity`: the caller's batch size - a short last batch must not rebuild)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if self.tta and not halves:                       # B-frame tensors: copied into the first halves of 2B-frame buffers
            src = (d_bgr, d_depth, d_masks)
            d_bgr, d_depth, d_masks = self.tta_alloc(B, H, W, d_masks.shape[1], d_depth is not None)
            for buf, t in zip((d_bgr, d_depth, d_masks), src):
                if t is not None:
                    buf[:B].copy_(t)
        # (nms and perturb write the caller's masks, unless they have just been copied); may_stop=False: always the fixed count, nothing
        # is read back here
        rec = self.device_pass(eng, d_bgr, d_depth, d_masks, d_scores, B, may_stop=False, own=n_masks, slots=slots, gt=gt)
        pinned = torch.zeros((2, B), dtype=torch.int32).pin_memory()                   # instance counts, refine_converged_at
        rec.count, rec.conv, rec.e0, rec.e1 = pinned[0], pinned[1], e0, e1
        rec.count.copy_(rec.post["count"], non_blocking=True)
        if rec.it is not None:
            rec.conv.copy_(rec.it["conv"], non_blocking=True)
        if rec.nm is not None:                            # each frame's own initial masks: the NMS's count, read at collect_batch
            rep = torch.zeros((B, 4), dtype=torch.int32).pin_memory()
            rep.copy_(rec.nm["report"], non_blocking=True)
            rec.own = rep[:, 0]
        if rec.ls is not None:                            # the loss records: valid once e1 has passed
            pin = torch.zeros(tuple(rec.ls["rec"].shape), dtype=torch.float64).pin_memory()
            pin.copy_(rec.ls["rec"], non_blocking=True)
            rec.ls["host"] = pin.numpy()
        e1.record()
        eng._in_flight = getattr(eng, "_in_flight", 0) + 1
        return rec

    def collect_batch(self, hd, host_masks=False):
        """-> (list of the reference's per-frame output dicts, device milliseconds of the whole batch[, per-frame numpy masks]).
        host_masks: also the refined masks of every frame as numpy bool [K_b, H, W] - what the reference's caller takes with
        output['instances'].to('cpu').pred_masks.numpy() - through ONE device-to-host copy for the whole batch (the arrays of a
        batch are views of one host block)."""
        hd.e1.synchronize()
        eng, post, count, conv = hd.eng, hd.post, hd.count.numpy(), hd.conv.numpy()
        kmax = int(count.max()) if len(count) else 0
        ready = hd.e1
        masks = hd.masks
        if kmax > hd.slots:                          # rare: more instances than pre-extracted slots - extracted now, on the caller's stream
            masks = eng.extract_masks(post, kmax)
            ready = torch.cuda.Event()
            ready.record()
        outs = [self.frame_dict(hd, b, int(count[b]), masks[b, :int(count[b])].view(torch.bool) if count[b] > 0 else None, conv[b])
                for b in range(len(count))]
        ms = hd.e0.elapsed_time(hd.e1)
        eng._in_flight = max(0, getattr(eng, "_in_flight", 1) - 1)
        if not host_masks:
            self._release_retired(eng)
            return outs, ms
        if kmax == 0:
            self._release_retired(eng)
            return outs, ms, [[] for _ in count]
        # The copy runs on a stream of its own, behind this batch's end event only: on the caller's stream it would queue behind
        # the NEXT batch, which predict_stream has already enqueued - and the host would wait 33 ms for masks that are ready.
        side = self._copy_stream()
        side.wait_event(ready)
        with torch.cuda.stream(side):
            host = masks[:, :kmax].contiguous().cpu().numpy().view(np.bool_)
        self._release_retired(eng)
        return outs, ms, [host[b, :int(count[b])] if count[b] > 0 else [] for b in range(len(count))]

    def _release_retired(self, eng):
        """An engine that a larger one has replaced and whose last batch in flight has just been collected: closed now.  (The tensors in
        the dicts collect_batch returned are torch allocations the engine wrote INTO - logits, post tables, masks - not buffers of the
        engine's context, so closing it invalidates nothing the caller holds.)"""
        if getattr(eng, "_in_flight", 0) > 0:
            return
        for key, lst in list(self._retired.items()):
            if eng in lst:
                lst.remove(eng)
                torch.cuda.synchronize(self.device)
                eng.close()
            if not lst:
                self._retired.pop(key, None)

    def close(self):
        """Release every engine (plan buffers, workspaces, weights in kernel layout) this model holds."""
        torch.cuda.synchronize(self.device)
        for lst in self._retired.values():
            for e in lst:
                e.close()
        for e in self._engines.values():
            e.close()
        if self._zoom_model is not None:
            self._zoom_model.close()
            self._zoom_model = None
        self._retired.clear()
        self._engines.clear()
        self._staging.clear()

    def _copy_stream(self):
        st = getattr(self, "_d2h_stream", None)
        if st is None:
            st = self._d2h_stream = torch.cuda.Stream(device=self.device)
        return st

    def __call__(self, batched_inputs):
        dev = self.device
        imgs = torch.stack([x["image"] for x in batched_inputs]).to(dev)
        offs = torch.stack([x["initial_pred_offset"] for x in batched_inputs]).to(dev, torch.float32).contiguous()
        nch = 3 * qconfig.arch_kwargs(self.cfg)["streams"]
        if imgs.shape[1] != nch:
            raise ValueError(f"expected a {nch}-channel image, got {imgs.shape[1]}")
        hwc = imgs.to(torch.uint8).permute(0, 2, 3, 1)
        bgr = hwc[..., :3].contiguous()
        depth = hwc[..., 3:].contiguous() if nch == 6 else None
        eng = self.engine_for(bgr.shape[1], bgr.shape[2], len(bgr))
        logits = eng.forward(bgr, depth, offs)                  # ready-made offsets: no initial masks, so nothing to count, track or perturb
        post = self.postprocess(eng, logits)
        return self.results(PassResult(eng, len(bgr), logits, post, err=self.decode(eng, logits)))


class MaskRefinerPredictor:
    def __init__(self, config_file=None, dataset_name="uoais_sim_val_panoptic", weights_file=None, device="cuda:0",
                 seed=0, state_dict=None, tta=False, decode_errors=False, iterations=1, until_converged=False, track_initial=False,
                 cleanup=None, perturb=None, nms=None, zoom=None, losses=None, cluster=None, scene=None, options=None, seeding=None, region=None):
        # the options (module docstring), checked before anything is loaded; options: a RefineOptions in their place
        # seeding: None or a quber_amd.seeding.DepthSeeding - nothing is imported, allocated or launched for it without one
        if seeding is not None:
            from ..seeding import DepthSeeding
            if not isinstance(seeding, DepthSeeding):
                raise ValueError(f"seeding={seeding!r}: expected None or a quber_amd.seeding.DepthSeeding")
        self.seeding = seeding
        # region: None or a quber_amd.region.RegionRefinement - likewise
        if region is not None:
            from ..region import RegionRefinement
            if not isinstance(region, RegionRefinement):
                raise ValueError(f"region={region!r}: expected None or a quber_amd.region.RegionRefinement")
            if not isinstance(cluster if options is None else options.cluster, GaussianMeanShift):
                raise ValueError("region: the Region Refinement Network refines the masks of cluster=GaussianMeanShift()")
        self.region = region
        self.options = options or RefineOptions.parse(tta=tta, decode_errors=decode_errors, iterations=iterations, until_converged=until_converged,
                                                      track_initial=track_initial, cleanup=cleanup, perturb=perturb, nms=nms, zoom=zoom,
                                                      losses=losses, cluster=cluster, scene=scene)
        vars(self).update(vars(self.options))
        if config_file is None:
            self.cfg = qconfig.canonical_cfg()
        else:
            self.cfg = qconfig.merge_from_file(qconfig.get_cfg(), config_file)
        qconfig.validate(self.cfg)
        self.depth_on = self.cfg.INPUT.DEPTH_ON
        self.rgb_on = self.cfg.INPUT.RGB_ON
        self.input_format = self.cfg.INPUT.FORMAT
        assert self.input_format in ["RGB", "BGR"], self.input_format
        self.sigma = 10
        kw = qconfig.arch_kwargs(self.cfg)
        path = weights_file
        if path is not None and not os.path.exists(path) and config_file is not None:
            # the reference derives the path from the config location (predictor.py:222-225)
            path = config_file.replace(".yaml", "/{}".format(weights_file)).replace("configs", "output")
        if state_dict is not None:                       # weights handed over in memory (bench / tests)
            sd, path = state_dict, "<state_dict>"
        elif path is not None and os.path.exists(path):
            sd = load_checkpoint(path)
        else:
            if weights_file is not None:
                warnings.warn(f"weights '{weights_file}' not found; using seeded synthetic weights")
            sd = arch.init_state_dict(seed=seed, **kw)
        self.cfg.MODEL.WEIGHTS = path or "<synthetic seed %d>" % seed
        self.model = RefinerModel(self.cfg, sd, device, options=self.options)
        self.device = torch.device(device)
        self.fast_path = os.environ.get("QUBER_PREDICT_FAST", "1") != "0"     # 0: the general batched path for single frames too

    # -- reference signature (predictor.py:287) --
    def predict(self, rgb_img, depth_img=None, perturbed_masks=None, mask_scores=None, gt_labels=None, embeddings=None, depth_z=None,
                center_votes=None, fg=None, proposals=None, xyz=None, camera=None):
        # camera (with seeding=, in place of xyz): a quber_amd.camera.Camera; depth_z (f32 [H,W], metres) is back-projected on the device
        # xyz (with seeding= and cluster=GaussianMeanShift(), in place of center_votes / fg): f32 [H,W,3] or [3,H,W], the organised point cloud
        # gt_labels (with losses=): the frame's ground-truth label map, integer [H,W], 0 = none, 1..n; the dict then carries `losses`
        # embeddings (with cluster=, in place of perturbed_masks): f32 [64,H,W]; depth_z: f32 [H,W], the depth filter's plane
        # center_votes, fg (with cluster=GaussianMeanShift(), in place of perturbed_masks): f32 [3,H,W] = xyz + offsets, and u8 / bool [H,W]
        if self.cluster is not None or embeddings is not None or depth_z is not None or center_votes is not None or fg is not None or xyz is not None or camera is not None:
            if perturbed_masks is not None:
                raise ValueError("cluster: embeddings= / center_votes= / xyz= take the place of the initial masks; both were given")
            if mask_scores is not None:
                raise ValueError("cluster: the clustering's masks have no scores; mask_scores= was given")
            return self.predict_batch(rgb_img[None], None if depth_img is None else depth_img[None], None,
                                      gt_labels=None if gt_labels is None else [gt_labels],
                                      embeddings=None if embeddings is None else [embeddings], depth_z=None if depth_z is None else [depth_z],
                                      center_votes=None if center_votes is None else [center_votes], fg=None if fg is None else [fg],
                                      xyz=None if xyz is None else [xyz], camera=camera)
        masks = np.zeros((0,) + rgb_img.shape[:2], np.uint8) if perturbed_masks is None else np.asarray(perturbed_masks)
        gts = None if gt_labels is None else [gt_labels]
        if self.scene is not None or proposals is not None:      # the general path; proposals (with scene=): u8 / bool [P,H,W], may be absent
            return self.predict_batch(rgb_img[None], None if depth_img is None else depth_img[None], [masks],
                                      None if mask_scores is None else [mask_scores], gt_labels=gts,
                                      proposals=None if proposals is None else [proposals])
        if self.nms is not None:                          # the general path: how many masks there are is known on the device only
            return self.predict_batch(rgb_img[None], None if depth_img is None else depth_img[None], [masks], [mask_scores], gt_labels=gts)
        if self.zoom is not None:                         # the general path: it keeps the frame on the device for the crops
            return self.predict_batch(rgb_img[None], None if depth_img is None else depth_img[None], [masks])
        if not self.fast_path or masks.dtype not in (np.uint8, np.bool_) or masks.ndim != 3:
            return self.predict_batch(rgb_img[None], None if depth_img is None else depth_img[None], [masks], gt_labels=gts)
        if self.depth_on and depth_img is None:
            raise ValueError("this config has INPUT.DEPTH_ON: a depth image is required")
        if not self.rgb_on:                               # depth-only: the image IS the depth map (predictor.py:296-298)
            rgb_img, depth_img = depth_img, None
        elif not self.depth_on:
            depth_img = None
        return [self.model.predict_one(rgb_img, depth_img, mask_bytes(masks, self.perturb is not None), gt_labels)]

    def _gms_inputs(self, B, H, W, center_votes, fg):
        """cluster=GaussianMeanShift(): the checked host arrays (votes f32 [B,3,H,W], fg u8 [B,H,W]) of a call."""
        if center_votes is None or fg is None or len(center_votes) != B or len(fg) != B:
            raise ValueError("cluster: center_votes= and fg= of every frame are required when cluster= is a GaussianMeanShift")
        votes = np.ascontiguousarray(np.stack([np.asarray(v) for v in center_votes]), dtype=np.float32)
        if votes.shape != (B, 3, H, W):
            raise ValueError(f"cluster: center_votes of shape {votes.shape[1:]} per frame, expected (3, {H}, {W})")
        on = np.stack([np.asarray(f) for f in fg])
        if on.shape != (B, H, W) or on.dtype not in (np.uint8, np.bool_):
            raise ValueError(f"cluster: fg of shape {on.shape[1:]} and dtype {on.dtype} per frame, expected ({H}, {W}) of uint8 or bool")
        if not np.isfinite(votes).all():
            raise ValueError("cluster: center_votes must be finite")
        if self.cluster.imp is not None and imp_plane_bytes(H, W) > IMP_LDS_BYTES:
            raise ValueError(f"cluster: the IMP's two bit planes of a {H} x {W} frame do not fit the LDS; there is no global-memory fallback")
        return votes, np.ascontiguousarray((on != 0).astype(np.uint8))

    def _xyz_inputs(self, B, H, W, xyz, masks_list, scores_list, embeddings, depth_z, center_votes, fg):
        """seeding=: the checked point clouds of a call as one device tensor f32 [B,3,H,W], before anything is launched; None without xyz=."""
        if xyz is None:
            return None
        if self.seeding is None:
            raise ValueError("xyz= needs seeding= (a quber_amd.seeding.DepthSeeding)")
        if not isinstance(self.cluster, GaussianMeanShift):
            raise ValueError("xyz: the Depth Seeding Network's votes go to cluster=GaussianMeanShift(); this predictor has " +
                             ("no cluster=" if self.cluster is None else "a MeanShift"))
        if center_votes is not None or fg is not None:
            raise ValueError("xyz: the network makes the votes and the foreground; center_votes= / fg= were given as well")
        if embeddings is not None or depth_z is not None:
            raise ValueError("cluster: a GaussianMeanShift takes xyz= or center_votes= and fg=, not embeddings= / depth_z=")
        if masks_list is not None:
            raise ValueError("xyz: the clustering makes the initial masks; masks were given as well")
        if scores_list is not None:
            raise ValueError("cluster: the clustering's masks have no scores; scores_list= was given")
        if len(xyz) != B:
            raise ValueError(f"xyz: the point clouds of {len(xyz)} frames for a batch of {B}")
        if H % 16 or W % 16:
            raise ValueError(f"xyz: the Depth Seeding Network needs a height and width that are multiples of 16, not {H} x {W}")
        if self.cluster.imp is not None and imp_plane_bytes(H, W) > IMP_LDS_BYTES:
            raise ValueError(f"cluster: the IMP's two bit planes of a {H} x {W} frame do not fit the LDS; there is no global-memory fallback")
        from ..seeding import as_xyz_batch
        return as_xyz_batch(list(xyz), H, W, self.device)

    def _camera_inputs(self, B, H, W, camera, xyz, masks_list, scores_list, embeddings, depth_z, center_votes, fg):
        """seeding= with camera=: the checked depth planes of a call as one device tensor f32 [B,H,W] (metres), before anything is
        launched; None without camera=.  The Depth Seeding Network's first op back-projects them (csrc/dsn.hip xyz_from_depth_kernel)."""
        if camera is None:
            return None
        from ..camera import Camera, check_depth_z
        if not isinstance(camera, Camera):
            raise ValueError(f"camera={camera!r}: expected a quber_amd.camera.Camera")
        if self.seeding is None:
            raise ValueError("camera= needs seeding= (a quber_amd.seeding.DepthSeeding)")
        if not isinstance(self.cluster, GaussianMeanShift):
            raise ValueError("camera: the Depth Seeding Network's votes go to cluster=GaussianMeanShift(); this predictor has " +
                             ("no cluster=" if self.cluster is None else "a MeanShift"))
        if xyz is not None:
            raise ValueError("camera: the point cloud comes from depth_z=; xyz= was given as well")
        if center_votes is not None or fg is not None:
            raise ValueError("camera: the network makes the votes and the foreground; center_votes= / fg= were given as well")
        if embeddings is not None:
            raise ValueError("cluster: a GaussianMeanShift takes camera= and depth_z=, xyz= or center_votes= and fg=, not embeddings=")
        if masks_list is not None:
            raise ValueError("camera: the clustering makes the initial masks; masks were given as well")
        if scores_list is not None:
            raise ValueError("cluster: the clustering's masks have no scores; scores_list= was given")
        if depth_z is None:
            raise ValueError("camera: depth_z= of every frame (f32 [H,W], metres) is required beside camera=")
        if len(depth_z) != B:
            raise ValueError(f"camera: the depth planes of {len(depth_z)} frames for a batch of {B}")
        if H % 16 or W % 16:
            raise ValueError(f"camera: the Depth Seeding Network needs a height and width that are multiples of 16, not {H} x {W}")
        if self.cluster.imp is not None and imp_plane_bytes(H, W) > IMP_LDS_BYTES:
            raise ValueError(f"cluster: the IMP's two bit planes of a {H} x {W} frame do not fit the LDS; there is no global-memory fallback")
        z = np.stack([check_depth_z(d, H, W, "camera: depth_z of frame %d" % b) for b, d in enumerate(depth_z)])
        return torch.from_numpy(z).to(self.device)

    def _region_z(self, B, H, W, seed_x, depth_z):
        """region=: the checked z planes of a call before anything is launched - depth_z= as a host array f32 [B,H,W], or the point clouds
        xyz= themselves (f32 [B,3,H,W] on the device: plane 2 is taken when the pass is enqueued); None without region=."""
        if self.region is None:
            return None
        if self.region.final_close_morphology and imp_plane_bytes(H, W) > IMP_LDS_BYTES:
            raise ValueError(f"region: the two bit planes of a {H} x {W} frame that final_close_morphology works on do not fit the LDS")
        if seed_x is not None:
            return seed_x
        if depth_z is None or len(depth_z) != B:
            raise ValueError("region: depth_z= of every frame (f32 [H,W]) is required beside center_votes= / fg=; with seeding= it is plane 2 of xyz=")
        z = np.ascontiguousarray(np.stack([np.asarray(d) for d in depth_z]), dtype=np.float32)
        if z.shape != (B, H, W):
            raise ValueError(f"region: depth_z of shape {z.shape[1:]} per frame, expected ({H}, {W})")
        return z

    def _seed(self, x, camera=None):
        """xyz f32 [B,3,H,W] on the device (with camera=: z f32 [B,H,W]) -> (votes, fg, first, draws) for Engine.gms, all on the device, the
        class map u8 [B,H,W] and the class counts i64 [B,3] (host).  One D2H of 3 B + 1 integers: the draw of a frame's first seed needs its
        foreground count."""
        from ..uois_chain import seed_stage
        return seed_stage(self.seeding, self.cluster, x, camera)

    def _scene_inputs(self, B, H, W, proposals):
        """scene=: the checked proposals of a call -> (u8 [B,P,H,W] with P = the longest list, zero rows behind a frame's own; their
        counts), before anything is uploaded or launched; None without scene=."""
        if self.scene is None:
            if proposals is not None:
                raise ValueError("proposals= needs scene= (a quber_amd.scene.ScenePerturb)")
            return None
        if proposals is None:
            proposals = [np.zeros((0, H, W), np.uint8)] * B
        if len(proposals) != B:
            raise ValueError(f"scene: proposals of {len(proposals)} frames for a batch of {B}")
        arrs = []
        for b, p in enumerate(proposals):
            p = np.zeros((0, H, W), np.uint8) if p is None else np.asarray(p)
            if p.ndim != 3 or p.shape[1:] != (H, W) or p.dtype not in (np.uint8, np.bool_):
                raise ValueError(f"scene: the proposals of frame {b} have shape {p.shape} and dtype {p.dtype}, expected (P, {H}, {W}) of uint8 or bool")
            arrs.append(p)
        out = np.zeros((B, max(len(p) for p in arrs), H, W), np.uint8)
        for b, p in enumerate(arrs):
            out[b, :len(p)] = p != 0
        return out, [len(p) for p in arrs]

    def _cluster_inputs(self, B, H, W, masks_list, scores_list, embeddings, depth_z, center_votes=None, fg=None):
        """cluster=: the checked host arrays (embeddings f32 [B,64,H,W], depth_z f32 [B,H,W] or None) of a call, before anything is
        uploaded or launched; None without cluster=.  The first seeds are drawn by the caller once every other check has passed."""
        ms = self.cluster
        if ms is None:
            if embeddings is not None or depth_z is not None:
                raise ValueError("embeddings= / depth_z= need cluster= (a quber_amd.meanshift.MeanShift)")
            if center_votes is not None or fg is not None:
                raise ValueError("center_votes= / fg= need cluster= (a quber_amd.gms.GaussianMeanShift)")
            return None
        if masks_list is not None:
            raise ValueError("cluster: embeddings= / center_votes= take the place of the initial masks; both were given")
        if scores_list is not None:
            raise ValueError("cluster: the clustering's masks have no scores; scores_list= was given")
        if isinstance(ms, GaussianMeanShift):
            if embeddings is not None or (depth_z is not None and self.region is None):
                raise ValueError("cluster: a GaussianMeanShift takes center_votes= and fg=, not embeddings= / depth_z=")
            return self._gms_inputs(B, H, W, center_votes, fg)
        if center_votes is not None or fg is not None:
            raise ValueError("cluster: a MeanShift takes embeddings=, not center_votes= / fg=")
        if embeddings is None or len(embeddings) != B:
            raise ValueError("cluster: the embeddings of every frame are required when cluster= is set")
        emb = np.ascontiguousarray(np.stack([np.asarray(e) for e in embeddings]), dtype=np.float32)
        if emb.shape != (B, CLUSTER_CHANNELS, H, W):
            raise ValueError(f"cluster: embeddings of shape {emb.shape[1:]} per frame, expected ({CLUSTER_CHANNELS}, {H}, {W})")
        if ms.num_seeds > H * W:
            raise ValueError("cluster: more seeds than the frame has pixels")
        z = None
        if ms.depth_threshold is not None:
            if depth_z is None or len(depth_z) != B:
                raise ValueError("cluster: depth_z of every frame is required when depth_threshold is set")
            z = np.ascontiguousarray(np.stack([np.asarray(d) for d in depth_z]), dtype=np.float32)
            if z.shape != (B, H, W):
                raise ValueError(f"cluster: depth_z of shape {z.shape[1:]} per frame, expected ({H}, {W})")
        return emb, z

    def predict_batch(self, rgb_imgs, depth_imgs, masks_list, scores_list=None, gt_labels=None, embeddings=None, depth_z=None,
                      center_votes=None, fg=None, proposals=None, xyz=None, camera=None):
        """rgb_imgs/depth_imgs: u8 [B,H,W,3] arrays; masks_list: B arrays u8/bool [N_b,H,W]; scores_list (required with nms=): B arrays
        [N_b] of finite scores; gt_labels (with losses=): the B ground-truth label maps, integer [B,H,W] or a list.  With cluster=:
        masks_list is None, embeddings: B arrays f32 [64,H,W], depth_z: B arrays f32 [H,W] (with depth_threshold); or, with a
        GaussianMeanShift, center_votes: B arrays f32 [3,H,W] and fg: B arrays u8 / bool [H,W] - or, with seeding=, xyz: B point clouds f32
        [H,W,3] / [3,H,W] in their place, or camera= (a quber_amd.camera.Camera) and depth_z: B depth planes f32 [H,W] in metres, back-projected on
        the device.  With scene=: masks_list holds every frame's
        GROUND TRUTH and proposals (optional) B arrays u8 / bool [P_b,H,W], the pool of segment proposals.  -> list of B dicts."""
        B, H, W = rgb_imgs.shape[:3]
        props = self._scene_inputs(B, H, W, proposals)
        seed_z = self._camera_inputs(B, H, W, camera, xyz, masks_list, scores_list, embeddings, depth_z, center_votes, fg)
        seed_x = seed_z if seed_z is not None else self._xyz_inputs(B, H, W, xyz, masks_list, scores_list, embeddings, depth_z, center_votes, fg)
        seeded = None
        # (with xyz=: a placeholder until the network has run, below, once every other check has passed)
        cluster_in = () if seed_x is not None else self._cluster_inputs(B, H, W, masks_list, scores_list, embeddings, depth_z, center_votes, fg)
        gms = isinstance(self.cluster, GaussianMeanShift)
        region_z = self._region_z(B, H, W, seed_x, depth_z)
        # rows of the mask tensor per frame; with cluster=: one plane per cluster there can be - the seeds' labels but the largest (a
        # GaussianMeanShift: a label per seed, each with min_pixels pixels of the frame)
        if cluster_in is None:
            counts = [len(m) for m in masks_list]
        elif gms:
            from ..uois_chain import mask_rows
            counts = [mask_rows(self.cluster, H, W)] * B
        else:
            counts = [min(max(self.cluster.num_seeds - 1, 1), 254)] * B
        sc = None
        if self.nms is not None:                          # checked before anything is uploaded or launched
            if scores_list is None or len(scores_list) != len(masks_list):
                raise ValueError("nms: the scores of every frame's masks are required when nms= is set")
            sc = np.full((B, max([len(m) for m in masks_list] + [1])), np.nan, np.float32)      # NaN: no such mask (a frame with fewer)
            for b, (m, s) in enumerate(zip(masks_list, scores_list)):
                sc[b, :len(m)] = check_scores(s, len(m), "the scores of frame %d" % b)
        if self.depth_on and depth_imgs is None:
            raise ValueError("this config has INPUT.DEPTH_ON: a depth image is required")
        if not self.rgb_on:                               # depth-only: the image IS the depth map (predictor.py:296-298)
            rgb_imgs, depth_imgs = depth_imgs, None
        elif not self.depth_on:
            depth_imgs = None
        n = max(counts + [1])
        n_rows = n if self.scene is None else self.scene.max_masks       # the mask rows of the pass
        if props is not None and n + props[0].shape[1] > SCENE_MAX_SLOTS:
            raise ValueError(f"scene: {n} ground-truth rows and {props[0].shape[1]} proposal rows: more than {SCENE_MAX_SLOTS} in all")
        mk = np.zeros((B, n, H, W) if cluster_in is None else (0,), np.uint8)
        for b, m in enumerate(masks_list if cluster_in is None else ()):
            if len(m):
                mk[b, :len(m)] = mask_bytes(m, self.perturb is not None or self.nms is not None, binarise=True)
        model = self.model
        gt = model.upload_gt(gt_labels, B, H, W)
        eng = model.engine_for(H, W, 2 * B if self.tta else B, max(n, n_rows, gt[2]) if gt is not None else max(n, n_rows))
        # uploaded straight into B-frame tensors (tta: the first halves of the 2B-frame buffers)
        bgr, depth, d_masks = model.batch_buffers(B, H, W, n_rows, depth_imgs is not None)
        bgr[:B].copy_(torch.from_numpy(np.ascontiguousarray(rgb_imgs, dtype=np.uint8)))
        if depth is not None:
            depth[:B].copy_(torch.from_numpy(np.ascontiguousarray(depth_imgs, dtype=np.uint8)))
        scene_in = None
        if self.scene is not None:                        # the uploaded masks are the scene's ground truth, in a tensor of their own
            i32 = lambda v: torch.from_numpy(np.asarray(v, np.int32)).to(self.device)
            scene_in = (torch.from_numpy(mk).to(self.device), i32(counts), torch.from_numpy(props[0]).to(self.device), i32(props[1]))
        elif cluster_in is None:
            d_masks[:B].copy_(torch.from_numpy(mk))
        else:                                             # the first seeds: drawn last, so that a call that raised above has drawn nothing
            if seed_x is not None:
                cluster_in, *seeded = self._seed(seed_x, camera)
            elif gms:
                first, draws = self.cluster.draws([self.cluster.n_sub(int(f.sum())) for f in cluster_in[1]])
                cluster_in = (cluster_in[0], cluster_in[1], first, draws.view(np.int32))
            else:
                cluster_in = (cluster_in[0], self.cluster.first_seeds(B, H * W), cluster_in[1])
            if seed_x is None:
                cluster_in = tuple(None if a is None else torch.from_numpy(a).to(self.device) for a in cluster_in)
        rec = model.device_pass(eng, bgr, depth, d_masks, None if sc is None else torch.from_numpy(sc).to(self.device), B, may_stop=True,
                                own=counts, gt=gt, cluster_in=cluster_in, scene_in=scene_in,
                                region_in=None if self.region is None else (
                                    self.region, seed_z if seed_z is not None else seed_x[:, 2].contiguous() if seed_x is not None else
                                    torch.from_numpy(region_z).to(self.device)))
        outs = model.results(rec, (bgr, depth))
        if seeded is not None:
            for b, r in enumerate(outs):
                r["seeding_fg"], r["seeding_report"] = seeded[0][b], torch.from_numpy(seeded[1][b].astype(np.int64))
        return outs
