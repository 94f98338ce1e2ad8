"""GPU: the per-frame half of COCO AP on the device (csrc/cocoap.hip through quber_amd.eval.coco_ap.CocoAP) against its numpy contract
(tests/test_cocoap_cpu.py).  Integers, bits and float64 expressions rounded operation by operation: every comparison is exact, float64
by bits; every byte of every output section is compared, so a call that left a byte of an earlier call behind fails."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from quber_amd import synth
from quber_amd.eval import coco_ap
from quber_amd.eval.coco_ap import ABSENT, CocoAP
from test_cocoap_cpu import (AREA_RNG, IOU_THRS, coco_accumulate_np, coco_frame_np, coco_stats_np, coco_summarize_np, example_a, rect)

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(ROOT, "quber_amd", "csrc", "cocoap.hip")).read()
CHUNK = int(re.search(r"constexpr int CA_CHUNK = (\d+);", _SRC).group(1))       # words of a bit plane per gram block
TOP = int(re.search(r"constexpr int CA_TOP = (\d+);", _SRC).group(1))
FILL = 0x3C


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    torch.cuda.synchronize()
    coco_ap.close_engines()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        a, b = bits(a), bits(b)
    assert np.array_equal(a, b), (what, a, b)


class Batch:
    """A padded batch as quber_coco_match takes it: scores NaN / flags 0xFF mark the slots that are not there."""

    def __init__(self, dt, scores, gt, flags=None, areas=None, dt_boxes=None, gt_boxes=None):
        self.dt, self.scores, self.gt = np.asarray(dt, np.uint8), np.asarray(scores, np.float32), np.asarray(gt, np.uint8)
        B, n_gt = self.gt.shape[:2]
        self.flags = np.zeros((B, n_gt), np.uint8) if flags is None else np.asarray(flags, np.uint8)
        self.areas, self.dt_boxes, self.gt_boxes = areas, dt_boxes, gt_boxes

    def args(self):
        return (self.dt, self.scores, self.gt), dict(gt_flags=self.flags, gt_areas=self.areas, dt_boxes=self.dt_boxes, gt_boxes=self.gt_boxes)

    def frame(self, b):
        """Frame b as the contract takes it (the present slots only), and their input indices."""
        pd, pg = np.flatnonzero(~np.isnan(self.scores[b])), np.flatnonzero(self.flags[b] != ABSENT)
        fr = {"dt": self.dt[b][pd], "scores": self.scores[b][pd], "gt": self.gt[b][pg], "crowd": (self.flags[b][pg] & 1) != 0,
              "ignore": (self.flags[b][pg] & 2) != 0}
        if self.areas is not None:
            fr["gt_area"] = self.areas[b][pg]
        if self.dt_boxes is not None:
            fr["dt_boxes"] = self.dt_boxes[b][pd]
        if self.gt_boxes is not None:
            fr["gt_boxes"] = self.gt_boxes[b][pg]
        return fr, pd, pg


def check_record(r, batch, iou_type="segm"):
    """Every byte of the sections `r` of one call against the contract on `batch`."""
    B, n_gt = batch.gt.shape[:2]
    A, T = len(AREA_RNG), len(IOU_THRS)
    for b in range(B):
        fr, pd, pg = batch.frame(b)
        iou, da, ga, recs = coco_frame_np(fr, iou_type)
        order = np.argsort(-fr["scores"], kind="mergesort")[:TOP]
        nt, ngp = len(order), len(pg)
        same(r["counts"][b], [nt, ngp], "counts")
        assert (recs[0] is None) == (nt == 0 and ngp == 0)
        same(r["order"][b], np.concatenate([pd[order], -np.ones(TOP - nt, np.int64)]).astype(np.int32), "order")
        same(r["scores"][b], np.concatenate([fr["scores"][order], np.zeros(TOP - nt, np.float32)]), "scores")
        same(r["dt_area"][b], np.concatenate([da[order], np.zeros(TOP - nt)]), "dt_area")
        want = np.zeros(n_gt)
        want[pg] = ga
        same(r["gt_area"][b], want, "gt_area")
        want = np.zeros((TOP, n_gt))
        want[:nt, pg] = iou[order].reshape(nt, ngp)
        same(r["iou"][b], want, "iou")                   # compared first: what the matching below is built on
        absent = np.setdiff1d(np.arange(n_gt), pg)
        for a in range(A):
            rec = recs[a]
            gi = np.full(n_gt, 2, np.uint8)
            dtm, dtig = np.zeros((T, TOP), np.uint8), np.zeros((T, TOP), np.uint8)
            gorder = absent
            if rec is not None:
                gi[pg] = rec["gi"]
                gorder = np.concatenate([pg[rec["gorder"]], absent])
                dtm[:, :nt], dtig[:, :nt] = rec["dtm"], rec["dtIg"]
                same(rec["scores"], r["scores"][b, :nt], "record scores")
            same(r["gi"][b, a], gi, ("gi", a))
            same(r["gorder"][b, a], gorder.astype(np.int32), ("gorder", a))
            same(r["dtm"][b, a], dtm, ("dtm", b, a))
            same(r["dtIg"][b, a], dtig, ("dtIg", b, a))


def run(batch, iou_type="segm", buf=None):
    ap = CocoAP(iou_type)
    args, kw = batch.args()
    hd = ap.enqueue(*args, buf=buf, **kw)
    r = ap.collect(hd)
    check_record(r, batch, iou_type)
    return ap, r


def noisy_rects(rng, n, h, w, p=0.03):
    m = np.stack([rect(h, w, rng.integers(0, h // 2), rng.integers(0, w // 2), rng.integers(3, h // 2), rng.integers(3, w // 2)) for _ in range(n)])
    return m ^ (rng.random(m.shape) < p).astype(np.uint8)


def general_batch():
    """37 x 70: a ragged last word, rows that are not 16-byte aligned; a duplicated detection and a duplicated ground truth (equal IoU rows
    and columns), equal scores, a NaN detection, an absent, a crowd and an ignored ground truth, the areas of one frame given."""
    rng = np.random.default_rng(11)
    B, n_dt, n_gt, h, w = 3, 7, 5, 37, 70
    gt = np.stack([noisy_rects(rng, n_gt, h, w, 0.01) for _ in range(B)])
    dt = np.stack([np.concatenate([np.roll(g, 2, 2)[:4] ^ (rng.random((4, h, w)) < 0.03), noisy_rects(rng, n_dt - 4, h, w)]) for g in gt]).astype(np.uint8)
    dt[0, 3], gt[0, 2] = dt[0, 1], gt[0, 0]
    dt[1, 5] = gt[1, 4]
    scores = rng.random((B, n_dt)).astype(np.float32)
    scores[0, 1] = scores[0, 3] = scores[0, 6] = 0.5
    scores[1, 2] = np.nan
    scores[2, :] = 0.25
    flags = np.zeros((B, n_gt), np.uint8)
    flags[0, 4], flags[1, 1], flags[1, 3], flags[2, 0] = 1, ABSENT, 2, 3
    areas = np.full((B, n_gt), np.nan)
    areas[1] = [5000., 7., 900., 1024., 10000.]
    areas[2, 3] = 1025.
    return Batch(dt * 255, scores, gt, flags, areas)


def empty_batch():
    """(0 detections, 3 ground truths), (4, 0), (0, 0) and a frame one of whose detections is an all-zero mask, in one batch."""
    rng = np.random.default_rng(12)
    B, n_dt, n_gt, h, w = 4, 4, 3, 37, 70
    gt, dt = np.stack([noisy_rects(rng, n_gt, h, w) for _ in range(B)]), np.stack([noisy_rects(rng, n_dt, h, w) for _ in range(B)])
    scores = rng.random((B, n_dt)).astype(np.float32)
    flags = np.zeros((B, n_gt), np.uint8)
    scores[0], flags[1], scores[2], flags[2] = np.nan, ABSENT, np.nan, ABSENT
    dt[3, 1] = 0
    scores[3, 1] = 2.0                                   # ranked first, IoU 0 with everything
    return Batch(dt, scores, gt, flags)


def test_general():
    run(general_batch())


def test_area_edges():
    h, w = 100, 130
    sizes = [1023, 1024, 1025, 9215, 9216, 9217]
    m = np.zeros((len(sizes), h * w), np.uint8)
    for i, s in enumerate(sizes):
        m[i, :s] = 1
    m = m.reshape(1, len(sizes), h, w)
    ap, r = run(Batch(m, np.linspace(.9, .4, len(sizes), dtype=np.float32)[None], m))
    same(r["dt_area"][0, :6], np.array(sizes, np.float64), "areas")
    # inclusive at both ends: 1024 is small and medium, 9216 medium and large
    assert r["gi"][0, 1].tolist() == [0, 0, 1, 1, 1, 1] and r["gi"][0, 2].tolist() == [1, 0, 0, 0, 0, 1] and r["gi"][0, 3].tolist() == [1, 1, 1, 1, 0, 0]


def test_iou_on_a_threshold():
    h, w = 9, 40                                         # one pair per row: the ground truth u pixels, the detection its first i
    pairs = [(3, 6), (3, 4), (9, 10), (19, 20), (2, 6), (2, 4), (8, 10), (18, 20)]
    gt, dt = np.zeros((8, h, w), np.uint8), np.zeros((8, h, w), np.uint8)
    for k, (i, u) in enumerate(pairs):
        gt[k, k, :u], dt[k, k, :i] = 1, 1
    ap, r = run(Batch(dt[None], np.linspace(.9, .2, 8, dtype=np.float32)[None], gt[None]))
    same(np.diagonal(r["iou"][0, :8]), np.array([np.float64(i) / np.float64(u) for i, u in pairs]), "iou")
    dtm = r["dtm"][0, 0]                                 # [T][rank]; rank k = pair k
    assert dtm[0, 0] == 1 and dtm[1, 0] == 0             # 3/6 at .50, not at .55
    assert dtm[5, 1] == 1 and dtm[6, 1] == 0             # 3/4 at .75
    assert IOU_THRS[8] < 0.9 and dtm[8, 2] == 1 and dtm[9, 2] == 0      # 9/10 at iouThrs[8] = 0.8999999999999999
    assert dtm[9, 3] == 1                                # 19/20 at .95
    assert dtm[0, 4] == 0 and dtm[5, 5] == 0 and dtm[0, 5] == 1 and dtm[8, 6] == 0 and dtm[5, 6] == 1 and dtm[9, 7] == 0 and dtm[8, 7] == 1


def test_more_than_100_detections():
    rng = np.random.default_rng(13)
    B, n_dt, n_gt, h, w = 2, 130, 12, 24, 40
    gt = np.stack([np.stack([rect(h, w, 6 * (k // 4), 10 * (k % 4), 6, 10) for k in range(n_gt)])] * B)
    dt = np.zeros((B, n_dt, h, w), np.uint8)
    for b in range(B):
        for d in range(n_dt):
            k = rng.integers(0, n_gt)
            dt[b, d] = rect(h, w, 6 * (k // 4) + rng.integers(0, 2), 10 * (k % 4) + rng.integers(0, 3), rng.integers(3, 7), rng.integers(5, 11))
    scores = rng.permutation(n_dt * B).reshape(B, n_dt).astype(np.float32) / (n_dt * B)
    by_rank = np.argsort(-scores[0], kind="mergesort")
    scores[0, by_rank[98:101]] = scores[0, by_rank[98]]  # ranks 99 - 101 (1-based) are equal: the lower index gets the last place
    scores[1, rng.permutation(n_dt)[:40]] = np.nan
    ap, r = run(Batch(dt, scores, gt))
    assert r["counts"][:, 0].tolist() == [100, 90]
    assert r["order"][0, 98:100].tolist() == sorted(by_rank[98:101].tolist())[:2]


def test_empty_frames():
    ap, r = run(empty_batch())
    assert r["counts"].tolist() == [[0, 3], [4, 0], [0, 0], [4, 3]]
    assert [rec is None for rec in ap.records[0]] == [False, False, True, False]
    assert r["order"][3, 0] == 1 and r["dt_area"][3, 0] == 0 and not r["iou"][3, 0].any()
    # no detection slot and no ground-truth slot at all
    e = np.zeros((2, 0, 37, 70), np.uint8)
    b = empty_batch()
    run(Batch(e, np.zeros((2, 0), np.float32), b.gt[:2]))
    run(Batch(b.dt[:2], b.scores[:2], e))
    ap, r = run(Batch(e, np.zeros((2, 0), np.float32), e))
    assert ap.summarize().tolist() == [-1] * 12


def test_gram_chunking():
    # rows of 64 pixels = 2 words (16-byte aligned rows: the 16-byte pack path); H = (CHUNK + 16) / 2 rows -> CHUNK + 16 words per plane,
    # a multiple of 4: the second gram chunk holds 16 words, a quarter of one staging slab
    h, w = (CHUNK + 16) // 2, 64
    assert h * (w // 32) == CHUNK + 16 and (CHUNK + 16) % 4 == 0
    rng = np.random.default_rng(14)
    B, n_dt, n_gt = 2, 100, 20
    gt = np.stack([np.stack([rect(h, w, (h // n_gt) * k, rng.integers(0, 20), h // n_gt + rng.integers(0, 9), rng.integers(20, 44)) for k in range(n_gt)])
                   for _ in range(B)])
    gt[:, -1, -3:, :] = 1                                # pixels in the last words of the plane
    dt = np.stack([np.stack([np.roll(gt[b, d % n_gt], (rng.integers(-6, 7), rng.integers(-4, 5)), (0, 1)) for d in range(n_dt)]) for b in range(B)])
    run(Batch(dt, rng.random((B, n_dt)).astype(np.float32), gt))


def test_bbox():
    # fractional boxes; detection 1 touches ground truth 0 at x = 2.5 (w == 0); ground truth 2 is a crowd
    db = np.array([[[0., 0., 2.5, 2.], [2.5, 0., 1.25, 1.], [1.125, 3.5, 40.75, 30.5], [0.1, 0.2, 0.3, 0.7]]])
    gb = np.array([[[0.5, 0.5, 2., 2.], [1., 3., 41., 33.3], [0., 0., 100., 100.], [0.1, 0.2, 0.3, 0.7]]])
    z = np.zeros((1, 4, 8, 8), np.uint8)
    ap, r = run(Batch(z, np.array([[.9, .8, .7, .6]], np.float32), z, flags=np.array([[0, 0, 1, 0]], np.uint8), dt_boxes=db, gt_boxes=gb), "bbox")
    assert r["iou"][0, 1, 0] == 0.0 and r["iou"][0, 0, 0] > 0 and r["iou"][0, 0, 2] == 1.0      # (inside the crowd: i == dw dh)
    # without boxes: the tight box of every mask, an empty mask included
    b = general_batch()
    b.dt[0, 2] = 0
    run(b, "bbox")
    b.gt_boxes = np.random.default_rng(15).random((3, 5, 4)) * 30      # given for one side only
    run(b, "bbox")
    # both sides given: no mask pointer reaches the library
    b.dt_boxes = np.random.default_rng(16).random((3, 7, 4)) * 30
    ap = CocoAP("bbox")
    check_record(ap.collect(ap.enqueue(None, b.scores, None, gt_flags=b.flags, gt_areas=b.areas, dt_boxes=b.dt_boxes, gt_boxes=b.gt_boxes)), b, "bbox")
    with pytest.raises(ValueError):
        ap.enqueue(None, b.scores, b.gt, dt_boxes=None)
    with pytest.raises(ValueError):
        CocoAP("segm").enqueue(b.dt, b.scores, b.gt, dt_boxes=b.dt_boxes)


def test_more_frames_than_one_engine_call():
    """B = 37 > coco_ap.MAX_BATCH: three library calls (16 + 16 + 5 frames) into the sections of one record buffer, one copy back."""
    assert coco_ap.MAX_BATCH == 16
    rng = np.random.default_rng(17)
    B, n_dt, n_gt, h, w = 37, 6, 4, 20, 33
    gt = np.stack([noisy_rects(rng, n_gt, h, w, 0.01) for _ in range(B)])
    dt = np.stack([np.concatenate([np.roll(g, 1, 2), noisy_rects(rng, n_dt - n_gt, h, w)]) for g in gt])
    scores = rng.random((B, n_dt)).astype(np.float32)
    scores[rng.random((B, n_dt)) < 0.1] = np.nan
    flags = rng.choice(np.array([0, 0, 0, 1, 2, ABSENT], np.uint8), (B, n_gt))
    ap, r = run(Batch(dt, scores, gt, flags))
    assert ap.frames == B
    run(Batch(dt, scores, gt, flags), "bbox")


def test_second_call_overwrites():
    g, e = general_batch(), empty_batch()
    buf = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda")
    for batch in (g, e, g):                              # the same record buffer and the same workspace
        run(batch, buf=buf)
    for batch in (g, e, g):
        run(batch, "bbox", buf=buf)


def test_limits_are_errors():
    from quber_amd import _lib
    z = np.zeros((1, 1025, 8, 8), np.uint8)
    with pytest.raises(ValueError):
        CocoAP().enqueue(z, np.zeros((1, 1025), np.float32), z[:, :1])
    lib, eng = _lib.load(), coco_ap._engine(8, 8, torch.device("cuda:0"))
    ptr = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda").data_ptr()
    for n_dt, n_gt, T, A in ((1025, 1, 10, 4), (1, 1025, 10, 4), (1, 1, 17, 4), (1, 1, 10, 9)):
        rc = lib.quber_coco_match(eng.h, ptr, ptr, None, n_dt, ptr, ptr, None, None, n_gt, 1, 0, ptr, T, ptr, A, *([ptr] * 10), None)
        assert rc != 0 and b"outside" in lib.quber_last_error()
    torch.cuda.synchronize()


def test_end_to_end_summary():
    rng = np.random.default_rng(16)
    ap, frames = CocoAP(), []
    for B, n_dt, n_gt in ((1, 3, 2), (4, 9, 5), (2, 1, 7)):
        h, w = 120, 160
        gt = np.stack([np.stack([rect(h, w, rng.integers(0, 20), rng.integers(0, 40), rng.integers(10, 100), rng.integers(10, 120)) for _ in range(n_gt)])
                       for _ in range(B)])
        dt = np.stack([np.stack([np.roll(gt[b, d % n_gt], (rng.integers(-5, 6), rng.integers(-5, 6)), (0, 1)) for d in range(n_dt)]) for b in range(B)])
        scores = rng.random((B, n_dt)).astype(np.float32)
        flags = (rng.random((B, n_gt)) < 0.15).astype(np.uint8)
        batch = Batch(dt, scores, gt, flags)
        # device tensors in for one batch, numpy for the others
        if B == 4:
            ap.update(torch.from_numpy(dt).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(gt).cuda() != 0, gt_flags=flags)
        else:
            ap.update(dt, scores, gt, gt_flags=flags)
        frames += [batch.frame(b)[0] for b in range(B)]
    want = coco_stats_np(frames)
    assert (want[:3] > 0).all() and (want[:3] < 1).all()
    same(ap.summarize(), want, "stats")
    res = ap.results()
    assert list(res) == ["AP", "AP50", "AP75", "APs", "APm", "APl"] and res["AP"] == want[0] * 100


def test_example_a_and_label_map_ground_truth():
    fr = example_a()
    ap = CocoAP()
    ap.update(fr["dt"], fr["scores"], fr["gt"])          # one frame, no batch axis
    same(ap.summarize(), coco_stats_np([fr]), "example A")
    assert abs(ap.summarize()[0] - 0.4524752475247524) < 1e-12
    assert np.isnan(ap.results()["APl"])
    # the same ground truth as a label map (labels 3 and 9 -> ground truths 0 and 1), a second frame with one label
    lab = (fr["gt"][0] * 3 + fr["gt"][1] * 9).astype(np.int32)
    ap2 = CocoAP()
    ap2.update(np.stack([fr["dt"], fr["dt"]]), np.stack([fr["scores"], fr["scores"]]), torch.from_numpy(np.stack([lab, (lab == 9) * 5])).cuda())
    two = dict(fr, gt=fr["gt"][1:])
    same(ap2.summarize(), coco_stats_np([fr, two]), "label map")
    # a uint8 label map (an annotation PNG) is a label map too: the number of axes decides; masks of another dtype count as non-zero = inside
    ap3 = CocoAP()
    ap3.update(fr["dt"].astype(np.float32) * 0.5, fr["scores"], lab.astype(np.uint8))
    same(ap3.summarize(), coco_stats_np([fr]), "uint8 label map, float masks")
    with pytest.raises(ValueError):
        ap3.update(fr["dt"], fr["scores"], lab.astype(np.float32))
    # as many labels as compact_labels allows
    many = np.zeros((16, 32), np.int32)
    many.ravel()[:254] = np.arange(1, 255)
    ap4 = CocoAP()
    r = ap4.update(np.zeros((1, 16, 32), np.uint8), np.array([.5], np.float32), many)
    assert r["counts"].tolist() == [[1, 254]] and (r["gt_area"] == 1).all()


def test_validation_ap_equals_cocoap_by_hand(tmp_path):
    from PIL import Image
    from quber_amd import arch
    from quber_amd.eval.refiner_model import MaskRefiner, compact_labels, label_map_from_masks
    items, annos = [], []
    for i in range(2):
        sc = synth.make_scene(60 + i, 480, 640, 4)
        Image.fromarray(sc["rgb"][:, :, ::-1].copy()).save(tmp_path / f"rgb{i}.png")
        Image.fromarray(sc["depth"][:, :, 0].astype(np.uint16) * 5 + 300).save(tmp_path / f"depth{i}.png")
        annos.append(label_map_from_masks(sc["gt_masks"], (480, 640), np.uint8))
        items.append((str(tmp_path / f"rgb{i}.png"), str(tmp_path / f"depth{i}.png"), sc["masks"] != 0, None))
    ref = MaskRefiner(None, None, dataset="OSD")
    model = ref.refiner_predictor.model                              # random weights with loud heads: real instances come out
    model.state_dict = arch.init_state_dict(seed=0, loud_heads=True, center_bias=-1.68)
    model._engines.clear()
    got = ref.validation_ap(items, annos, workers=2, batch=2)
    assert got["n"] == 2
    init, refined = CocoAP(), CocoAP()
    for item, anno, res in zip(items, annos, ref.predict_stream(items, workers=2, batch=2)):
        gt = compact_labels(anno)
        init.update(item[2], np.ones(len(item[2]), np.float32), gt)
        inst = res[1]["instances"]
        refined.update(np.asarray(res[0]), inst.scores.cpu().numpy(), gt)
    same(got["initial"]["stats"], init.summarize(), "initial")
    same(got["refined"]["stats"], refined.summarize(), "refined")
    np.testing.assert_equal(got["refined"]["results"], refined.results())
    assert got["initial"]["stats"][0] > 0 and refined.frames == 2
