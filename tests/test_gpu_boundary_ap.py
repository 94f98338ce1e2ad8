"""GPU: Boundary AP on the device - the boundary kernel on its own (csrc/boundaryap.hip through Engine.mask_boundary) and the per-frame half
under Boundary IoU (quber_coco_match_boundary through CocoAP("boundary")) - against the numpy contract of tests/test_boundary_ap_cpu.py.
Bits, integers and one float64 division per ratio: every comparison is exact, float64 by bits; every byte of every output is compared and
every output sits between guard bands."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from quber_amd import _lib
from quber_amd.eval import coco_ap
from quber_amd.eval.coco_ap import ABSENT, CocoAP
from test_boundary_ap_cpu import blobs, coco_boundary_stats_np, coco_frame_boundary_np, hand_example, mask_boundary_np
from test_cocoap_cpu import AREA_RNG, IOU_THRS, coco_stats_np, rect
from test_gpu_cocoap import FILL, TOP, Batch, check_record, noisy_rects, same

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(ROOT, "quber_amd", "csrc", "boundaryap.hip")).read()
BAND = int(re.search(r"constexpr int CB_BAND = (\d+);", _SRC).group(1))         # rows of a plane per workgroup
COLS = int(re.search(r"constexpr int CB_COLS = (\d+);", _SRC).group(1))         # words of a row per workgroup
GUARD = 4096


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    torch.cuda.synchronize()
    coco_ap.close_engines()


def engine():
    return coco_ap._engine(8, 8, torch.device("cuda:0"))   # the op takes its frame size per call


def guarded(shape, dtype):
    """A device tensor of `shape` between two guard bands of FILL bytes -> (the whole buffer as bytes, the view)."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes].view(dtype).view(shape)


def guards_intact(whole):
    h = whole.cpu().numpy()
    return (h[:GUARD] == FILL).all() and (h[-GUARD:] == FILL).all()


def mask_set(rng, h, w, n=17):
    """Masks touching each edge, all four at once, the full frame, one pixel in each corner, none, a one-pixel hole, random blobs."""
    ms = [rect(h, w, 0, w // 4, max(1, h // 2), max(1, w // 2)), rect(h, w, h - max(1, h // 2), w // 4, max(1, h // 2), max(1, w // 2)),
          rect(h, w, h // 4, 0, max(1, h // 2), max(1, w // 2)), rect(h, w, h // 4, w - max(1, w // 2), max(1, h // 2), max(1, w // 2)),
          rect(h, w, 0, w // 3, h, max(1, w // 3)) | rect(h, w, h // 3, 0, max(1, h // 3), w), np.ones((h, w), np.uint8)]
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        one = np.zeros((h, w), np.uint8)
        one[y, x] = 1
        ms.append(one)
    ms.append(np.zeros((h, w), np.uint8))
    hole = np.ones((h, w), np.uint8)
    hole[h // 2, w // 2] = 0
    ms.append(hole)
    while len(ms) < n:
        ms.append(blobs(rng, h, w, (0.9, 0.97, 0.999)[len(ms) % 3]))
    return np.stack(ms[:n]) * np.uint8(255)


def check_op(masks, d, out_whole=None, out=None):
    """One call of the op against the contract: bytes, areas, guard bands."""
    n, h, w = masks.shape
    if out is None:
        out_whole, out = guarded((n, h, w), torch.uint8)
    area_whole, area = guarded((n, 2), torch.int32)
    got, got_area = engine().mask_boundary(torch.from_numpy(masks).cuda(), d, out=out, area=area)
    want = np.stack([mask_boundary_np(m, d) for m in masks]).astype(np.uint8) if n else np.zeros((0, h, w), np.uint8)
    same(got.cpu().numpy(), want, ("boundary", h, w, d))
    same(got_area.cpu().numpy(), np.stack([(masks != 0).reshape(n, -1).sum(1), want.reshape(n, -1).sum(1)], 1).astype(np.int32), ("area", h, w, d))
    assert guards_intact(out_whole) and guards_intact(area_whole), (h, w, d)


# ---- the kernel on its own ----
@pytest.mark.parametrize("d", [1, 2, 16, 31, 32, 33, 64])
def test_mask_boundary_shapes(d):
    """The window inside one word, exactly one word, across two words, wider than the row (2d + 1 > W) and taller than the frame."""
    rng = np.random.default_rng(100 + d)
    for h in (3, 37, 70):
        for w in (5, 32, 33, 64, 70, 150):
            check_op(mask_set(rng, h, w), d)


@pytest.mark.parametrize("h", [BAND - 1, BAND, BAND + 1, 2 * BAND + 3])
def test_mask_boundary_band_edges(h):
    rng = np.random.default_rng(200 + h)
    for d in (1, 16, 64):
        check_op(mask_set(rng, h, 70), d)


def test_mask_boundary_column_tiles():
    """A row of more than CB_COLS words: the second column tile reads its neighbours across the tile edge."""
    w = 32 * COLS + 70
    rng = np.random.default_rng(300)
    for d in (2, 33):
        check_op(mask_set(rng, 5, w, 14), d)


def test_mask_boundary_counts():
    rng = np.random.default_rng(400)
    for n in (1, 17, 120):
        check_op(np.stack([blobs(rng, 37, 53, 0.97) for _ in range(n)]), 2)
    eng = engine()
    out, area = eng.mask_boundary(torch.zeros((0, 37, 53), dtype=torch.uint8, device="cuda"), 2)
    assert out.shape == (0, 37, 53) and area.shape == (0, 2)
    # in place
    m = torch.from_numpy(mask_set(rng, 37, 53)).cuda()
    want = np.stack([mask_boundary_np(x, 3) for x in m.cpu().numpy()]).astype(np.uint8)
    got, _ = eng.mask_boundary(m, 3, out=m)
    same(got.cpu().numpy(), want, "in place")


def test_mask_boundary_dilation_limits_write_nothing():
    masks = torch.from_numpy(mask_set(np.random.default_rng(500), 37, 53)).cuda()
    out_whole, out = guarded(tuple(masks.shape), torch.uint8)
    area_whole, area = guarded((len(masks), 2), torch.int32)
    for d in (0, 65, -1):
        with pytest.raises(_lib.QuberError, match="dilation outside 1..64"):
            engine().mask_boundary(masks, d, out=out, area=area)
    torch.cuda.synchronize()
    assert (out_whole.cpu().numpy() == FILL).all() and (area_whole.cpu().numpy() == FILL).all()


def test_mask_boundary_second_call_overwrites():
    rng = np.random.default_rng(600)
    out_whole, out = guarded((17, 37, 70), torch.uint8)
    for k, d in enumerate((16, 2, 16)):
        check_op(mask_set(rng, 37, 70) if k != 1 else np.stack([blobs(rng, 37, 70) for _ in range(17)]), d, out_whole, out)


# ---- the per-frame half under Boundary IoU ----
def check_record_boundary(r, batch, d):
    """Every byte of the sections `r` of one "boundary" call against the contract on `batch`."""
    B, n_gt = batch.gt.shape[:2]
    A, T = len(AREA_RNG), len(IOU_THRS)
    for b in range(B):
        fr, pd, pg = batch.frame(b)
        iou, iou_m, iou_b, da, ga, recs = coco_frame_boundary_np(fr, d)
        order = np.argsort(-fr["scores"], kind="mergesort")[:TOP]
        nt, ngp = len(order), len(pg)
        same(r["counts"][b], [nt, ngp], "counts")
        same(r["order"][b], np.concatenate([pd[order], -np.ones(TOP - nt, np.int64)]).astype(np.int32), "order")
        same(r["scores"][b], np.concatenate([fr["scores"][order], np.zeros(TOP - nt, np.float32)]), "scores")
        same(r["dt_area"][b], np.concatenate([da[order], np.zeros(TOP - nt)]), "dt_area")       # the mask areas
        want = np.zeros(n_gt)
        want[pg] = ga
        same(r["gt_area"][b], want, "gt_area")
        for name, table in (("mask_iou", iou_m), ("boundary_iou", iou_b), ("iou", iou)):        # each on its own, then their minimum
            want = np.zeros((TOP, n_gt))
            want[:nt, pg] = table[order].reshape(nt, ngp)
            same(r[name][b], want, (name, b))
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
            same(r["gi"][b, a], gi, ("gi", a))
            same(r["gorder"][b, a], gorder.astype(np.int32), ("gorder", a))
            same(r["dtm"][b, a], dtm, ("dtm", b, a))
            same(r["dtIg"][b, a], dtig, ("dtIg", b, a))


def run_boundary(batch, d, buf=None, **kw):
    ap = CocoAP("boundary", **kw)
    args, kwargs = batch.args()
    r = ap.collect(ap.enqueue(*args, buf=buf, **kwargs))
    check_record_boundary(r, batch, d)
    return ap, r


def ragged_batch(h, w, seed):
    """3 frames with 7 / 6 / 2 detections and 5 / 3 / 5 ground truths: NaN scores and ABSENT slots as padding, two crowds, an ignored
    ground truth, equal scores, a duplicated detection, given areas in one frame."""
    rng = np.random.default_rng(seed)
    B, n_dt, n_gt = 3, 7, 5
    gt = np.stack([noisy_rects(rng, n_gt, h, w, 0.01) for _ in range(B)])
    dt = np.stack([np.concatenate([np.roll(g, 1, 2)[:4] ^ (rng.random((4, h, w)) < 0.01), noisy_rects(rng, n_dt - 4, h, w)]) for g in gt]).astype(np.uint8)
    dt[0, 3] = dt[0, 1]
    dt[1, 5] = gt[1, 4]
    dt[2, 0] = gt[2, 2]
    scores = rng.random((B, n_dt)).astype(np.float32)
    scores[0, 1] = scores[0, 3] = 0.5
    scores[1, 2] = np.nan
    scores[2, 2:] = np.nan
    flags = np.zeros((B, n_gt), np.uint8)
    flags[0, 4], flags[0, 1], flags[1, 1], flags[1, 3], flags[2, 0] = 1, 1, ABSENT, ABSENT, 2
    areas = np.full((B, n_gt), np.nan)
    areas[2] = [5000., 7., np.nan, 1024., 10000.]
    return Batch(dt * 255, scores, gt, flags, areas)


def test_hand_example_boundary_differs_from_segm():
    fr, d = hand_example()
    batch = Batch(fr["dt"][None], fr["scores"][None], fr["gt"][None])
    ap_b, rb = run_boundary(batch, d, dilation=d)
    ap_s = CocoAP("segm")
    rs = ap_s.collect(ap_s.enqueue(*batch.args()[0]))
    check_record(rs, batch)
    assert rb["mask_iou"][0, 0, 0] == 600 / 748 and rb["boundary_iou"][0, 0, 0] == 60 / 332 and rb["iou"][0, 0, 0] == 60 / 332
    assert rs["dtm"][0, 0, :7, 0].all() and not rb["dtm"][0].any()         # matched up to .80 under segm, at no threshold under boundary
    assert rb["dt_area"][0, 0] == 748 and rb["gt_area"][0, 0] == 600
    same(ap_b.summarize(), coco_boundary_stats_np([fr], d), "stats")
    assert ap_s.summarize()[1] > 0.99 and ap_b.summarize()[1] == 0
    assert list(ap_b.results()) == list(ap_s.results())


def test_ragged_batches_and_the_ratio_rule():
    b = ragged_batch(37, 53, 21)
    ap, r = run_boundary(b, 2, dilation=2)
    same(ap.summarize(), coco_boundary_stats_np([b.frame(k)[0] for k in range(3)], 2), "stats 37 x 53")
    assert (r["boundary_iou"] < r["mask_iou"]).any() and (r["iou"] > 0).any()
    # 70 x 150: the dilation distance from the frame's diagonal (3), more than one row band of the boundary kernel
    assert coco_ap.boundary_dilation(70, 150) == 3
    b = ragged_batch(70, 150, 22)
    ap, r = run_boundary(b, 3)
    same(ap.summarize(), coco_boundary_stats_np([b.frame(k)[0] for k in range(3)], 3), "stats 70 x 150")
    run_boundary(b, 6, dilation_ratio=0.036)
    run_boundary(b, 33, dilation=33)
    # frames without detections, without ground truths, without either
    e = np.zeros((2, 0, 37, 53), np.uint8)
    g = ragged_batch(37, 53, 23)
    run_boundary(Batch(e, np.zeros((2, 0), np.float32), g.gt[:2]), 2, dilation=2)
    run_boundary(Batch(g.dt[:2], g.scores[:2], e), 2, dilation=2)
    ap, r = run_boundary(Batch(e, np.zeros((2, 0), np.float32), e), 2, dilation=2)
    assert ap.summarize().tolist() == [-1] * 12
    with pytest.raises(ValueError):
        CocoAP("boundary").enqueue(g.dt, g.scores, g.gt, dt_boxes=np.zeros((3, 7, 4)))


def test_more_than_100_detections():
    rng = np.random.default_rng(24)
    B, n_dt, n_gt, h, w = 2, 130, 6, 37, 53
    gt = np.stack([np.stack([rect(h, w, 18 * (k // 3), 17 * (k % 3), 17, 16) for k in range(n_gt)])] * B)
    dt = np.zeros((B, n_dt, h, w), np.uint8)
    for b in range(B):
        for k in range(n_dt):
            g = rng.integers(0, n_gt)
            dt[b, k] = rect(h, w, 18 * (g // 3) + rng.integers(0, 2), 17 * (g % 3) + rng.integers(0, 2), rng.integers(14, 18), rng.integers(13, 17))
    scores = rng.permutation(n_dt * B).reshape(B, n_dt).astype(np.float32) / (n_dt * B)
    scores[1, rng.permutation(n_dt)[:40]] = np.nan
    ap, r = run_boundary(Batch(dt, scores, gt), 2, dilation=2)
    assert r["counts"][:, 0].tolist() == [100, 90] and (r["boundary_iou"] > 0).any()


def test_label_map_ground_truth():
    fr, d = hand_example()
    gt2 = np.stack([fr["gt"][0], rect(37, 53, 30, 40, 6, 12)])
    lab = (gt2[0] * 3 + gt2[1] * 9).astype(np.int32)
    ap = CocoAP("boundary", dilation=d)
    r = ap.update(fr["dt"], fr["scores"], torch.from_numpy(lab).cuda())
    same(ap.summarize(), coco_boundary_stats_np([dict(fr, gt=gt2)], d), "label map")
    assert r["boundary_iou"][0, 0, 0] == 60 / 332 and r["counts"].tolist() == [[1, 2]]


def test_mask_iou_equals_segm_and_segm_is_untouched():
    """dev_mask_iou of the new entry = dev_iou of quber_coco_match(iou_type 0), byte for byte; a "segm" run before and after a "boundary" run on
    the same engine and workspace writes identical bytes."""
    b = ragged_batch(70, 150, 25)
    args, kw = b.args()
    bufs = []
    for kind in ("segm", "boundary", "segm"):
        buf = torch.full((1 << 17,), FILL, dtype=torch.uint8, device="cuda")
        ap = CocoAP(kind)
        hd = ap.enqueue(*args, buf=buf, **kw)
        bufs.append((ap.collect(hd), hd.buf.cpu().numpy().copy()))
    (r0, raw0), (rb, _), (r1, raw1) = bufs
    assert np.array_equal(raw0, raw1)
    check_record(r0, b)
    assert rb["mask_iou"].tobytes() == r0["iou"].tobytes()
    assert rb["dt_area"].tobytes() == r0["dt_area"].tobytes() and rb["gt_area"].tobytes() == r0["gt_area"].tobytes()
    assert not np.array_equal(rb["iou"], r0["iou"])
    same(CocoAP("segm").update(*args, **kw)["iou"], r0["iou"], "segm again")


def test_second_call_overwrites_and_workspace():
    eng = coco_ap._engine(37, 53, torch.device("cuda:0"))
    g, h = ragged_batch(37, 53, 26), hand_example()[0]
    one = Batch(h["dt"][None], h["scores"][None], h["gt"][None])
    buf = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda")
    for batch in (g, one, g):                            # the same record buffer and the same workspace
        run_boundary(batch, 2, buf=buf, dilation=2)
    lib = _lib.load()
    segm, bnd = (lib.quber_debug_ws_bytes(1, 3, 5, 0, 37, 53, mode) for mode in (0, 2))
    planes = 3 * (TOP + 5) * ((37 * 2 + 3) // 4 * 4) * 4
    table = 3 * (TOP * 5 + TOP + 5) * 4
    up = lambda v: (v + 255) // 256 * 256
    assert bnd - segm == up(planes) + up(2 * table) - up(table)      # the boundary planes, the second pair table and the boundary areas
    assert eng.workspace_bytes() >= bnd


def test_limits_are_errors():
    lib, eng = _lib.load(), coco_ap._engine(8, 8, torch.device("cuda:0"))
    whole = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda")
    ptr = whole.data_ptr()

    def call(n_dt=1, n_gt=1, d=1, T=10, A=4):
        return lib.quber_coco_match_boundary(eng.h, ptr, ptr, n_dt, ptr, ptr, None, n_gt, 1, d, ptr, T, ptr, A, *([ptr] * 12), None)

    for kw in (dict(d=0), dict(d=65), dict(n_dt=1025), dict(n_gt=1025), dict(T=17), dict(A=9)):
        assert call(**kw) != 0 and b"outside" in lib.quber_last_error(), kw
    torch.cuda.synchronize()
    assert (whole.cpu().numpy() == FILL).all()
    with pytest.raises(ValueError):
        CocoAP("boundary", dilation_ratio=0.9).enqueue(np.zeros((1, 1, 70, 150), np.uint8), np.zeros((1, 1), np.float32), np.zeros((1, 1, 70, 150), np.uint8))


def test_stats_over_several_updates():
    rng = np.random.default_rng(27)
    ap, ap_s, frames = CocoAP("boundary"), CocoAP("segm"), []
    d = coco_ap.boundary_dilation(70, 150)
    for B, n_dt, n_gt in ((1, 3, 2), (4, 9, 5)):
        h, w = 70, 150
        gt = np.stack([np.stack([rect(h, w, rng.integers(0, 20), rng.integers(0, 40), rng.integers(10, 50), rng.integers(10, 100)) for _ in range(n_gt)])
                       for _ in range(B)])
        dt = np.stack([np.stack([np.roll(gt[b, k % n_gt], (rng.integers(-2, 3), rng.integers(-2, 3)), (0, 1)) for k in range(n_dt)]) for b in range(B)])
        scores = rng.random((B, n_dt)).astype(np.float32)
        batch = Batch(dt, scores, gt)
        ap.update(torch.from_numpy(dt).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(gt).cuda() != 0)
        ap_s.update(dt, scores, gt)
        frames += [batch.frame(b)[0] for b in range(B)]
    want = coco_boundary_stats_np(frames, d)
    same(ap.summarize(), want, "stats")
    same(ap_s.summarize(), coco_stats_np(frames), "segm stats")
    assert 0 < want[0] < ap_s.summarize()[0]             # shifted copies: the boundary measure is the stricter one
