"""The contract of Boundary AP (csrc/boundaryap.hip, csrc/cocoap.hip: quber_coco_match_boundary; quber_amd.eval.coco_ap.CocoAP("boundary")),
as numpy, and hand-derived cases that pin it.  It restates mask_to_boundary and COCOeval.computeBoundaryIoU of the published
boundary-iou-api (Cheng et al., "Boundary IoU") for one category: boundary(m) = m & ~erode_d(m) with zeros outside the frame, iou =
min(mask IoU, boundary IoU), everything behind the IoU table as in tests/test_cocoap_cpu.py.  The boundary_iou package, pycocotools and
cv2 are not available to these tests: parity with the package is argued (DESIGN.md "Boundary AP"), not pinned.  Everything here is exact:
integers, one float64 division, a min.  The GPU tests (tests/test_gpu_boundary_ap.py) compare the device with these functions bit for bit."""
import inspect

import numpy as np
import pytest
from scipy import ndimage

from test_cocoap_cpu import (AREA_RNG, IOU_THRS, coco_accumulate_np, coco_eval_img_np, coco_summarize_np, mask_iou_np, rect)


def boundary_dilation_np(h, w, ratio=0.02):
    return max(1, int(round(ratio * np.sqrt(np.float64(h * h + w * w)))))


def _run_and(a, d, axis):
    """out[i] = AND of a[i - d .. i + d] along `axis`, everything outside the array read as False: running sums, no shifted copies."""
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    c = np.concatenate([np.zeros((1,) + a.shape[1:], np.int64), np.cumsum(a, axis=0, dtype=np.int64)])
    out = np.zeros(a.shape, bool)
    if n >= 2 * d + 1:
        out[d:n - d] = (c[2 * d + 1:] - c[:n - 2 * d]) == 2 * d + 1
    return np.moveaxis(out, 0, axis)


def mask_boundary_np(m, d):
    """m [H,W] (non-zero = inside) -> bool [H,W]: m & ~erode_d(m); a pixel survives the erosion iff the (2d + 1) x (2d + 1) square around it
    lies inside the frame and inside m - a running AND along the rows, then along the columns."""
    m = np.asarray(m) != 0
    return m & ~_run_and(_run_and(m, d, 1), d, 0)


def boundary_iou_np(dt, gt, crowd, d):
    """-> (iou = min(mask iou, boundary iou) f64 [D,G], mask iou, boundary iou, dt areas, gt areas: the MASK areas)."""
    iou_m, da, ga = mask_iou_np(dt, gt, crowd)
    bd = np.array([mask_boundary_np(m, d) for m in dt]).reshape((len(dt),) + np.shape(dt)[1:])
    bg = np.array([mask_boundary_np(m, d) for m in gt]).reshape((len(gt),) + np.shape(gt)[1:])
    iou_b, _, _ = mask_iou_np(bd, bg, crowd)
    return np.minimum(iou_m, iou_b), iou_m, iou_b, da, ga


def coco_frame_boundary_np(frame, d, area_rng=AREA_RNG, iou_thrs=IOU_THRS):
    """coco_frame_np of tests/test_cocoap_cpu.py under Boundary IoU -> (iou, mask iou, boundary iou, dt_area, gt_area as used, records)."""
    crowd = np.asarray(frame.get("crowd", np.zeros(len(frame["gt"]))), bool)
    ignore = np.asarray(frame.get("ignore", np.zeros(len(frame["gt"]))), bool)
    iou, iou_m, iou_b, da, ga = boundary_iou_np(frame["dt"], frame["gt"], crowd, d)
    given = frame.get("gt_area")
    if given is not None:
        given = np.asarray(given, np.float64)
        ga = np.where(np.isnan(given), ga, given)
    recs = [coco_eval_img_np(frame["scores"], da, ga, crowd, ignore, iou, rng, iou_thrs) for rng in area_rng]
    return iou, iou_m, iou_b, da, ga, recs


def coco_boundary_stats_np(frames, d):
    records = [[] for _ in AREA_RNG]
    for fr in frames:
        for a, rec in enumerate(coco_frame_boundary_np(fr, d)[5]):
            records[a].append(rec)
    return coco_summarize_np(*coco_accumulate_np(records))


def blobs(rng, h, w, p=0.9):
    """A random blob mask: dense noise, so that erosions of several pixels leave something and holes of every size occur."""
    m = rng.random((h, w)) < p
    m[: h // 5] &= rng.random((h // 5, w)) < 0.5
    if h > 8 and w > 8:
        m[h // 3: h // 3 + 2 * (h // 4), w // 4: w // 4 + w // 2] = True
    return m.astype(np.uint8)


def hand_example():
    """37 x 53, d = 2.  Ground truth: the 20 x 30 rectangle at (8, 10), 600 px.  Detection: the 22 x 34 rectangle at (7, 8) - one row more
    above and below, two columns more left and right - 748 px, which holds the ground truth: mask IoU 600 / 748 = .802.  The boundaries are
    rings two pixels thick: 748 - 18 * 30 = 208 px and 600 - 16 * 26 = 184 px.  The detection's ring covers the rows 7 - 8 and 27 - 28 and the
    columns 8 - 9 and 40 - 41; the ground truth's the rows 8 - 9 and 26 - 27 and the columns 10 - 11 and 38 - 39.  They share row 8 and row
    27 over the ground truth's 30 columns: i_b = 60, boundary IoU 60 / (208 + 184 - 60) = .181."""
    h, w = 37, 53
    return {"dt": rect(h, w, 7, 8, 22, 34)[None], "scores": np.array([.9], np.float32), "gt": rect(h, w, 8, 10, 20, 30)[None]}, 2


# ---- the erosion ----
@pytest.mark.parametrize("h,w,d", [(7, 33, 1), (37, 53, 2), (40, 70, 3), (21, 100, 5), (64, 64, 16)])
def test_boundary_equals_iterated_erosion(h, w, d):
    rng = np.random.default_rng(h * 1000 + w)
    for k in range(6):
        m = blobs(rng, h, w, (0.8, 0.95, 0.995)[k % 3])
        if k == 5:
            m[:] = 1
        er = ndimage.binary_erosion(m != 0, np.ones((3, 3), bool), iterations=d, border_value=0)
        assert np.array_equal(mask_boundary_np(m, d), (m != 0) & ~er), (h, w, d, k)


def test_rectangles_closed_form():
    H, W = 40, 70
    for d in (1, 2, 5, 16):
        for (y0, x0, hh, ww) in ((6, 9, 20, 33), (0, 0, 20, 33), (20, 37, 20, 33), (0, 10, 40, 12), (3, 3, 2 * d, 40), (3, 3, 2 * d + 1, 2 * d + 1)):
            b = mask_boundary_np(rect(H, W, y0, x0, hh, ww), d)
            # zero border: touching the frame edge changes nothing
            assert int(b.sum()) == hh * ww - max(0, hh - 2 * d) * max(0, ww - 2 * d), (d, y0, x0, hh, ww)
            inner = rect(H, W, y0 + d, x0 + d, max(0, hh - 2 * d), max(0, ww - 2 * d)) if hh > 2 * d and ww > 2 * d else np.zeros((H, W), np.uint8)
            assert np.array_equal(b, (rect(H, W, y0, x0, hh, ww) != 0) & (inner == 0))
        full = mask_boundary_np(np.ones((H, W), np.uint8), d)
        assert int(full.sum()) == H * W - max(0, H - 2 * d) * max(0, W - 2 * d)
        one = np.zeros((H, W), np.uint8)
        one[0, W - 1] = 1
        assert np.array_equal(mask_boundary_np(one, d), one != 0)
        assert not mask_boundary_np(np.zeros((H, W), np.uint8), d).any()
    # H < 2d + 1: nothing survives the erosion, the boundary is the mask
    m = blobs(np.random.default_rng(3), 9, 60)
    assert np.array_equal(mask_boundary_np(m, 5), m != 0)
    assert mask_boundary_np(np.ones((11, 60), np.uint8), 5).sum() == 11 * 60 - 50
    # a one-pixel hole opens a (2d + 1)^2 square of boundary around it
    m = np.ones((31, 31), np.uint8)
    m[15, 15] = 0
    b = mask_boundary_np(m, 3)
    assert b[12:19, 12:19].sum() == 48 and not b[15, 15] and not b[11, 11:20].any()


def test_boundary_dilation():
    from quber_amd.eval.coco_ap import boundary_dilation
    for (h, w), d in (((480, 640), 16), ((720, 1280), 29), ((240, 320), 8), ((37, 53), 1)):
        assert boundary_dilation(h, w) == d == boundary_dilation_np(h, w)
    assert 0.02 * np.sqrt(37 * 37 + 53 * 53) > 0.5 and 0.005 * np.sqrt(37 * 37 + 53 * 53) < 0.5
    assert boundary_dilation(37, 53, 0.005) == 1          # round() gives 0: the floor of 1 holds
    assert boundary_dilation(70, 150, 0.02) == 3 and boundary_dilation(480, 640, 0.01) == 8


# ---- the IoU and the matching ----
def test_hand_example_segm_matches_boundary_does_not():
    fr, d = hand_example()
    iou, iou_m, iou_b, da, ga, recs = coco_frame_boundary_np(fr, d)
    assert da.tolist() == [748] and ga.tolist() == [600]             # the mask areas, not the rings'
    assert int(mask_boundary_np(fr["dt"][0], d).sum()) == 208 and int(mask_boundary_np(fr["gt"][0], d).sum()) == 184
    assert iou_m[0, 0] == 600 / 748 and iou_b[0, 0] == 60 / 332 and iou[0, 0] == 60 / 332
    assert iou_m[0, 0] >= 0.75 and iou_b[0, 0] < 0.5
    segm = coco_eval_img_np(fr["scores"], da, ga, [False], [False], iou_m, AREA_RNG[0])
    assert segm["dtm"][:, 0].tolist() == [t <= 600 / 748 for t in IOU_THRS] and segm["dtm"][5, 0]     # matched up to .80
    assert not recs[0]["dtm"].any() and not recs[0]["dtIg"].any()    # unmatched at every threshold: a false positive
    stats = coco_boundary_stats_np([fr], d)
    assert stats[0] == 0 and stats[8] == 0 and stats[3] == 0 and stats[4] == -1      # 600 px: small


def test_perfect_predictions():
    h, w = 120, 160
    gt = np.stack([rect(h, w, 0, 0, 20, 20), rect(h, w, 30, 0, 40, 50), rect(h, w, 0, 60, 100, 100)])
    for d in (1, 4, 16):
        stats = coco_boundary_stats_np([{"dt": gt.copy(), "scores": np.array([.9, .8, .7], np.float32), "gt": gt}], d)
        np.testing.assert_allclose(np.delete(stats, 6), np.ones(11), rtol=0, atol=1e-12)      # AP = AR100 = 1 (one ulp below: spacing(1))
        assert abs(stats[6] - 1 / 3) < 1e-15


def test_crowd_uses_detection_boundary_only():
    h, w, d = 30, 40, 2
    gt = rect(h, w, 0, 0, 30, 40)[None]                   # a crowd over the whole frame: its boundary is a ring at the frame edge
    dt = rect(h, w, 0, 5, 12, 10)[None]                   # touches the top edge
    iou, iou_m, iou_b, da, ga = boundary_iou_np(dt, gt, [True], d)
    bd, bg = mask_boundary_np(dt[0], d), mask_boundary_np(gt[0], d)
    i_b, db = int((bd & bg).sum()), int(bd.sum())
    assert db == 120 - 8 * 6 and i_b == 20                # of the detection's ring, the two top rows lie in the crowd's
    assert iou_m[0, 0] == 1.0 and iou_b[0, 0] == np.float64(i_b) / np.float64(db) and iou[0, 0] == iou_b[0, 0]
    not_crowd = boundary_iou_np(dt, gt, [False], d)
    assert not_crowd[2][0, 0] == np.float64(i_b) / np.float64(db + int(bg.sum()) - i_b) and not_crowd[1][0, 0] == 120 / 1200
    # disjoint boundaries of overlapping masks: boundary IoU 0, so the minimum is 0
    inner = rect(h, w, 10, 10, 6, 6)[None]
    assert boundary_iou_np(inner, gt, [False], d)[0][0, 0] == 0 and boundary_iou_np(inner, gt, [False], d)[1][0, 0] > 0


# ---- the host half of the package ----
def test_package_host_half():
    import torch
    from quber_amd import _lib
    from quber_amd.eval import coco_ap
    from quber_amd.eval.refiner_model import MaskRefiner
    assert coco_ap.MAX_DILATION == 64
    for bad in (dict(iou_type="boundary", dilation=0), dict(iou_type="boundary", dilation=65), dict(iou_type="boundary", dilation=2.5),
                dict(iou_type="boundary", dilation_ratio=0), dict(iou_type="boundary", dilation_ratio=float("nan")), dict(iou_type="contour")):
        with pytest.raises(ValueError):
            coco_ap.CocoAP(**bad)
    if not torch.cuda.is_available():                     # "boundary" is a known type: what is missing is the device, as for "segm"
        for kind in ("segm", "boundary"):
            with pytest.raises(_lib.QuberError):
                coco_ap.CocoAP(kind)
    sig = inspect.signature(coco_ap.CocoAP.__init__).parameters
    assert list(sig)[1:3] == ["iou_type", "device"] and sig["dilation_ratio"].default == 0.02 and sig["dilation"].default is None
    sig = inspect.signature(MaskRefiner.validation_ap).parameters
    assert list(sig)[:5] == ["self", "items", "anno_paths", "workers", "batch"]
    assert sig["boundary"].default is False and sig["dilation_ratio"].default == 0.02
    for name in ("quber_coco_match_boundary", "quber_op_mask_boundary"):
        assert name in _lib.SIGNATURES


def test_validation_ap_keys(monkeypatch):
    """boundary=False leaves validation_ap's dict as it was; True adds the two boundary entries (the device half replaced by a stand-in)."""
    from quber_amd.eval import coco_ap
    from quber_amd.eval.refiner_model import MaskRefiner
    made = []

    class Stub:
        def __init__(self, iou_type="segm", device=None, **kw):
            made.append((iou_type, kw))

        def summarize(self):
            return np.full(12, -1.0)

        def results(self):
            return {}

    class Predictor:
        device = "cpu"

    class Self:
        refiner_predictor = Predictor()

        def predict_stream(self, items, workers, batch):
            return iter(list(items))

    monkeypatch.setattr(coco_ap, "CocoAP", Stub)
    got = MaskRefiner.validation_ap(Self(), [], [])
    assert list(got) == ["initial", "refined", "n"] and got["n"] == 0 and made == [("segm", {}), ("segm", {})]
    del made[:]
    got = MaskRefiner.validation_ap(Self(), [], [], boundary=True, dilation_ratio=0.01)
    assert list(got) == ["initial", "refined", "initial_boundary", "refined_boundary", "n"]
    assert made[2:] == [("boundary", {"dilation_ratio": 0.01})] * 2
    assert list(got["initial_boundary"]) == list(got["initial"]) == ["stats", "results"]
