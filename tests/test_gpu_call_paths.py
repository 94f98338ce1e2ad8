"""GPU: the predictor's three call paths compute the same thing and launch the same work (quber_amd/maskrefiner/predictor.py).

``predict`` (batch 1, pinned staging), ``predict_batch`` and ``enqueue_batch`` + ``collect_batch`` (the stream) run one sequence on the
device and differ in who owns the buffers and where the host reads.  The per-option files compare them one option at a time; here
every option is on at once, on one seeded 96x128 scene with loud heads (tests/test_gpu_loud_parity.py: real instances):
  * one frame through all three: the same keys - the reference's, plus what the module docstring of predictor.py lists per option -
    and the same tensors, bit for bit; only ``scores`` get the allowance of test_gpu_iterate.py::_same_outputs (float64 atomic sums);
  * the same with ``nms`` (perturb off, so that the two do not mask one another) and with ``zoom`` (which the stream refuses);
  * two frames with 3 and 1 initial masks: which rows of the per-mask tables are a frame's own;
  * the public Engine methods every path calls, in order, against lists written out from the code.
Batch-2 results are never compared with batch-1 results: split-K partitions follow the launch size (tests/test_gpu_network.py)."""
import numpy as np
import pytest
import torch

from quber_amd.masknms import MaskNMS
from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
from quber_amd.perturb import Perturb
from quber_amd.zoom import ZoomIn
from test_gpu_loud_parity import _scene, loud_state_dict
from test_gpu_zoom import CROP

pytestmark = pytest.mark.gpu

H, W, N = 96, 128, 3
ALL = dict(tta=True, decode_errors=True, iterations=2, track_initial=True, cleanup="largest")
PERTURB = dict(perturb=Perturb(0.8, seed=3))

REFERENCE_KEYS = {"sem_seg", "eee_boundary", "panoptic_seg", "instances"}
OPTION_KEYS = {"eee_boundary_classes", "eee_boundary_hist",              # decode_errors (iterations > 1: no <head>_mask_hist)
               "refine_passes", "refine_converged_at",                    # iterations
               "initial_overlap"}                                         # track_initial
PERTURB_KEYS = {"perturbed_masks", "perturb_report"}
NMS_KEYS = {"nms_masks", "nms_source", "nms_scores", "nms_report"}
ZOOM_KEYS = {"coarse_instances", "zoom_ids", "zoom_rois", "zoom_report"}
INSTANCE_FIELDS = {"pred_masks", "scores", "pred_boxes", "pred_classes", "initial_index", "initial_iou",            # reference, track_initial
                   "cc_components", "cc_removed", "cc_filled"}                                                       # cleanup
ZOOMED_FIELDS = {"pred_masks", "scores", "pred_boxes", "pred_classes", "zoom_source"}

# the public Engine methods of one frame with ALL + PERTURB, as the code of each path calls them
FORWARD = ["perturb_masks", "tta_flip_inputs", "encode", "forward", "tta_merge", "postprocess", "cleanup_post",      # pass 1
           "relabel_panoptic", "encode_label_map", "forward", "tta_merge", "postprocess", "cleanup_post",            # pass 2
           "relabel_panoptic", "overlap_ids", "overlap_masks"]                                                       # its flags; track_initial
CALLS = {"predict": ["alloc_post"] + FORWARD + ["error_heads", "error_decode", "extract_masks"],      # (the first call builds the staging)
         "predict_batch": FORWARD + ["error_heads", "error_decode", "extract_masks"],
         "stream": FORWARD + ["extract_masks", "error_heads", "error_decode"]}         # the slots are extracted before anything is read

_CASE = []


def _case():
    """(batch of two frames with N masks each, loud weights), computed once and left unchanged."""
    if not _CASE:
        batch, offs, image = _scene(5, 2, H, W, N)
        _CASE.append((batch, loud_state_dict(2, image, offs, N)))
    return _CASE[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream(pred, rgb, dep, masks_list, scores_list=None, n_masks=None):
    """enqueue_batch + collect_batch on the frames as a caller of the stream uploads them: padded masks, NaN scores behind a frame's own."""
    n = max([len(m) for m in masks_list] + [1])
    pad = np.zeros((len(masks_list), n, H, W), np.uint8)
    sc = None if scores_list is None else np.full((len(masks_list), n), np.nan, np.float32)
    for b, m in enumerate(masks_list):
        pad[b, :len(m)] = m
        if sc is not None:
            sc[b, :len(m)] = scores_list[b]
    hd = pred.model.enqueue_batch(dev(rgb), dev(dep), dev(pad), n_masks=n_masks, d_scores=None if sc is None else dev(sc))
    return pred.model.collect_batch(hd)[0]


def _same_instances(a, b, fields, what):
    assert set(a.get_fields()) == set(b.get_fields()) == fields, (what, sorted(a.get_fields()), sorted(b.get_fields()))
    assert len(a) == len(b) >= 1, (what, "an instance per frame, or the comparison is blind")
    for f in fields:
        x, y = a.get(f), b.get(f)
        x, y = (x.tensor, y.tensor) if hasattr(x, "tensor") else (x, y)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, f)
        if f == "scores":            # post_paint_stats sums with float64 atomic adds: their order can move the last bit
            np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=2e-5, atol=1e-6, err_msg="%s: %s" % (what, f))
        else:
            assert torch.equal(x, y), (what, f)


def _same(a, b, keys, what, fields=INSTANCE_FIELDS, own=None):
    """Two output dicts of one frame: the key set `keys`, every value equal.  own: `a` comes from predict_batch, `b` from the stream,
    whose per-mask histograms keep the rows of the padding behind the frame's `own` masks (all zero)."""
    assert set(a) == set(b) == keys, (what, sorted(a), sorted(b))
    for key in sorted(keys):
        x, y = a[key], b[key]
        if key == "instances":
            _same_instances(x, y, ZOOMED_FIELDS if "zoom_ids" in keys else fields, "%s: %s" % (what, key))
        elif key == "coarse_instances":
            _same_instances(x, y, fields, "%s: %s" % (what, key))
        elif key == "panoptic_seg":
            assert x[1] is None and y[1] is None and torch.equal(x[0], y[0]), (what, key)
        elif key.endswith("_mask_hist") and own is not None:
            assert x.shape[0] == own and torch.equal(x, y[:own]) and not bool(y[own:].any()), (what, key)
        elif isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and torch.equal(x, y), (what, key)
        else:
            assert type(x) is type(y) and x == y, (what, key, x, y)


def _record(eng, calls):
    """Every public method of this Engine instance appends its name to `calls` when the predictor calls it (not when another Engine
    method does)."""
    depth = [0]

    def wrap(name, fn):
        def wrapped(*a, **kw):
            if depth[0] == 0:
                calls.append(name)
            depth[0] += 1
            try:
                return fn(*a, **kw)
            finally:
                depth[0] -= 1
        return wrapped
    for name in dir(eng):
        if not name.startswith("_") and callable(getattr(eng, name)):
            setattr(eng, name, wrap(name, getattr(eng, name)))


def test_all_options_one_frame_three_paths_same_dicts_same_launches():
    batch, sd = _case()
    rgb, dep, masks = batch["rgb"][0], batch["depth"][0], batch["masks"][0]
    pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, **ALL, **PERTURB)
    try:
        calls = []
        _record(pred.model.engine_for(H, W, 2, N), calls)       # the engine all three paths use: tta runs the frame and its mirror
        outs, seen = {}, {}
        for name, run in (("predict", lambda: pred.predict(rgb, dep, masks)[0]),
                          ("predict_batch", lambda: pred.predict_batch(rgb[None], dep[None], [masks])[0]),
                          ("stream", lambda: _stream(pred, rgb[None], dep[None], [masks])[0])):
            del calls[:]
            outs[name] = run()
            seen[name] = list(calls)
        keys = REFERENCE_KEYS | OPTION_KEYS | PERTURB_KEYS
        for name in ("predict_batch", "stream"):
            _same(outs["predict"], outs[name], keys, name)
        out = outs["predict"]
        assert out["refine_passes"] == 2 and tuple(out["initial_overlap"].shape) == (N, len(out["instances"]) + 1)
        assert tuple(out["perturbed_masks"].shape) == (N, H, W) and not np.array_equal(out["perturbed_masks"].cpu().numpy(), masks)
        for name in CALLS:
            assert seen[name] == CALLS[name], (name, seen[name])
    finally:
        pred.model.close()


def test_nms_one_frame_three_paths_same_dicts():
    batch, sd = _case()
    rgb, dep, masks = batch["rgb"][0], batch["depth"][0], batch["masks"][0]
    masks = np.concatenate([masks, np.roll(masks[:1], 2, axis=2)])          # a near copy of mask 0 with the lowest score: suppressed
    scores = np.array([0.9, 0.8, 0.7, 0.6], np.float32)
    pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, nms=MaskNMS(), **ALL)
    try:
        out = pred.predict(rgb, dep, masks, scores)[0]
        keys = REFERENCE_KEYS | OPTION_KEYS | NMS_KEYS
        _same(out, pred.predict_batch(rgb[None], dep[None], [masks], [scores])[0], keys, "predict_batch")
        _same(out, _stream(pred, rgb[None], dep[None], [masks], [scores])[0], keys, "stream")
        assert out["nms_report"].tolist() == [N, N] and sorted(out["nms_source"].tolist()) == [0, 1, 2]       # (listed in paint order)
        assert tuple(out["nms_masks"].shape) == (N, H, W) and tuple(out["initial_overlap"].shape) == (N, len(out["instances"]) + 1)
    finally:
        pred.model.close()


def test_zoom_one_frame_two_paths_same_dicts_and_the_stream_refuses():
    batch, sd = _case()
    rgb, dep, masks = batch["rgb"][0], batch["depth"][0], batch["masks"][0]
    pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, zoom=ZoomIn(crop=CROP), **ALL, **PERTURB)
    try:
        out = pred.predict(rgb, dep, masks)[0]
        keys = REFERENCE_KEYS | OPTION_KEYS | PERTURB_KEYS | ZOOM_KEYS
        _same(out, pred.predict_batch(rgb[None], dep[None], [masks])[0], keys, "predict_batch")
        assert int(out["zoom_report"][0]) == len(out["coarse_instances"]) and int(out["zoom_report"][3]) == len(out["instances"])
        with pytest.raises(ValueError, match="zoom"):
            pred.model.enqueue_batch(dev(rgb[None]), dev(dep[None]), dev(masks[None]))
    finally:
        pred.model.close()


def test_two_frames_with_3_and_1_masks_own_rows():
    batch, sd = _case()
    rgb, dep = batch["rgb"], batch["depth"]
    masks = [batch["masks"][0], batch["masks"][1][:1]]
    own = [len(m) for m in masks]
    opts = dict(ALL, iterations=1)                  # one pass: the per-mask histograms exist
    pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, **opts, **PERTURB)
    try:
        outs = pred.predict_batch(rgb, dep, masks)
        strm = _stream(pred, rgb, dep, masks, n_masks=own)
        keys = (REFERENCE_KEYS | OPTION_KEYS | PERTURB_KEYS | {"eee_boundary_mask_hist"}) - {"refine_passes", "refine_converged_at"}
        for b in range(2):
            _same(outs[b], strm[b], keys, "frame %d" % b, own=own[b])
            for o in (outs[b], strm[b]):
                assert o["initial_overlap"].shape[0] == own[b] and o["perturbed_masks"].shape[0] == own[b]
            # predict_batch trims the histogram to the frame's own masks; the stream keeps the N rows of the padded batch
            assert outs[b]["eee_boundary_mask_hist"].shape[0] == own[b] and strm[b]["eee_boundary_mask_hist"].shape[0] == N
    finally:
        pred.model.close()
