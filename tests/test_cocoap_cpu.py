"""The contract of the COCO AP path (csrc/cocoap.hip, quber_amd/eval/coco_ap.py), as numpy in plain loops, and hand-derived cases that
pin it.  It restates the published algorithm - COCOeval.computeIoU / evaluateImg / accumulate / summarize and bbIou / rleIou of
maskApi.c - for one category.  pycocotools is not available to these tests: parity with pycocotools is unpinned (DESIGN.md "COCO AP").
The GPU tests (tests/test_gpu_cocoap.py) compare the device records and the package's numbers with these functions bit for bit."""
import numpy as np
import pytest

IOU_THRS = np.linspace(.5, .95, int(np.round((.95 - .5) / .05)) + 1)
REC_THRS = np.linspace(0, 1, 101)
AREA_RNG = np.array([[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]], np.float64)
MAX_DETS = (1, 10, 100)


def mask_iou_np(dt, gt, crowd):
    """dt [D,H,W], gt [G,H,W] (non-zero = inside), crowd [G] -> (iou f64 [D,G], dt areas f64 [D], gt areas f64 [G])."""
    dt, gt = np.asarray(dt) != 0, np.asarray(gt) != 0
    iou = np.zeros((len(dt), len(gt)), np.float64)
    da = [int(m.sum()) for m in dt]
    ga = [int(m.sum()) for m in gt]
    for d in range(len(dt)):
        for g in range(len(gt)):
            i = int((dt[d] & gt[g]).sum())
            if i == 0:
                continue
            iou[d, g] = np.float64(i) / np.float64(da[d]) if crowd[g] else np.float64(i) / np.float64(da[d] + ga[g] - i)
    return iou, np.array(da, np.float64), np.array(ga, np.float64)


def box_iou_np(db, gb, crowd):
    """db [D,4], gb [G,4] float64 x, y, w, h -> (iou f64 [D,G], dt areas, gt areas)."""
    db, gb = np.asarray(db, np.float64).reshape(-1, 4), np.asarray(gb, np.float64).reshape(-1, 4)
    iou = np.zeros((len(db), len(gb)), np.float64)
    for d in range(len(db)):
        dx, dy, dw, dh = db[d]
        for g in range(len(gb)):
            gx, gy, gw, gh = gb[g]
            w = min(dx + dw, gx + gw) - max(dx, gx)
            h = min(dy + dh, gy + gh) - max(dy, gy)
            if w <= 0 or h <= 0:
                continue
            i = w * h
            u = dw * dh if crowd[g] else dw * dh + gw * gh - i
            iou[d, g] = i / u
    return iou, db[:, 2] * db[:, 3], gb[:, 2] * gb[:, 3]


def tight_boxes_np(masks):
    """[N,H,W] -> f64 [N,4]: x0, y0, x1 + 1 - x0, y1 + 1 - y0 (BitMasks.get_bounding_boxes as x, y, w, h); zeros for an empty mask."""
    out = np.zeros((len(masks), 4), np.float64)
    for n, m in enumerate(np.asarray(masks) != 0):
        ys, xs = np.nonzero(m)
        if len(ys):
            out[n] = xs.min(), ys.min(), xs.max() + 1 - xs.min(), ys.max() + 1 - ys.min()
    return out


def coco_eval_img_np(scores, dt_area, gt_area, crowd, ignore, iou, arng, iou_thrs=IOU_THRS, max_det=100):
    """COCOeval.evaluateImg of one frame and one area range.  scores f32 [D], dt_area [D], gt_area / crowd / ignore [G], iou f64 [D,G] in
    input order -> None for a frame with neither detections nor ground truths, else the record
    {order (input indices of the ranked detections), scores, dtm [T,nd], dtIg [T,nd], gi [G] (input order), gorder [G], gtIg = gi[gorder]}."""
    scores = np.asarray(scores, np.float32)
    D, G = len(scores), len(gt_area)
    if D == 0 and G == 0:
        return None
    order = np.argsort(-scores, kind="mergesort")[:max_det]
    gi = np.array([int(bool(ignore[g]) or bool(crowd[g]) or gt_area[g] < arng[0] or gt_area[g] > arng[1]) for g in range(G)], np.int64)
    gorder = np.argsort(gi, kind="mergesort")
    T, nd = len(iou_thrs), len(order)
    dtm, dtig, matched = np.zeros((T, nd), bool), np.zeros((T, nd), bool), np.zeros((T, G), bool)
    for ti, t in enumerate(iou_thrs):
        for di, d in enumerate(order):
            best, m = min(t, 1 - 1e-10), -1
            for g in gorder:
                if matched[ti, g] and not crowd[g]:
                    continue
                if m > -1 and gi[m] == 0 and gi[g] == 1:
                    break
                if iou[d, g] < best:
                    continue
                best, m = iou[d, g], g
            if m == -1:
                continue
            dtig[ti, di], dtm[ti, di], matched[ti, m] = bool(gi[m]), True, True
    for di, d in enumerate(order):
        out = bool(dt_area[d] < arng[0] or dt_area[d] > arng[1])
        for ti in range(T):
            dtig[ti, di] = dtig[ti, di] or (not dtm[ti, di] and out)
    return {"order": order, "scores": scores[order], "dtm": dtm, "dtIg": dtig, "gi": gi, "gorder": gorder, "gtIg": gi[gorder]}


def coco_accumulate_np(records, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS):
    """COCOeval.accumulate.  records[a]: the records of area range a over the frames (None entries are dropped)
    -> (precision [T,R,A,M], recall [T,A,M]), -1 where nothing can be said."""
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(records), len(max_dets)
    precision, recall = -np.ones((T, R, A, M)), -np.ones((T, A, M))
    for a in range(A):
        E = [e for e in records[a] if e is not None]
        if not E:
            continue
        for mi, md in enumerate(max_dets):
            scores = np.concatenate([e["scores"][:md] for e in E])
            inds = np.argsort(-scores, kind="mergesort")
            dtm = np.concatenate([e["dtm"][:, :md] for e in E], axis=1)[:, inds]
            dtig = np.concatenate([e["dtIg"][:, :md] for e in E], axis=1)[:, inds]
            npig = int(sum(int((np.asarray(e["gtIg"]) == 0).sum()) for e in E))
            if npig == 0:
                continue
            tps = np.logical_and(dtm, np.logical_not(dtig))
            fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
            for t in range(T):
                tp = np.cumsum(tps[t]).astype(float)
                fp = np.cumsum(fps[t]).astype(float)
                nd = len(tp)
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                recall[t, a, mi] = rc[-1] if nd else 0
                pr = pr.tolist()
                for i in range(nd - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                ix = np.searchsorted(rc, rec_thrs, side="left")
                q = np.zeros(R)
                for r in range(R):
                    if ix[r] >= nd:
                        break
                    q[r] = pr[ix[r]]
                precision[t, :, a, mi] = q
    return precision, recall


def _mean_valid(x):
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0


def coco_summarize_np(precision, recall):
    """COCOeval.summarize -> the twelve numbers: AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl (thresholds 0 and 5 of the ten are
    0.5 and 0.75; area ranges all, small, medium, large; the last entry of max_dets = 100)."""
    m = precision.shape[3] - 1
    return np.array([_mean_valid(precision[:, :, 0, m]), _mean_valid(precision[0, :, 0, m]), _mean_valid(precision[5, :, 0, m]),
                     _mean_valid(precision[:, :, 1, m]), _mean_valid(precision[:, :, 2, m]), _mean_valid(precision[:, :, 3, m]),
                     _mean_valid(recall[:, 0, 0]), _mean_valid(recall[:, 0, 1]), _mean_valid(recall[:, 0, 2]),
                     _mean_valid(recall[:, 1, m]), _mean_valid(recall[:, 2, m]), _mean_valid(recall[:, 3, m])], np.float64)


def coco_frame_np(frame, iou_type="segm", area_rng=AREA_RNG, iou_thrs=IOU_THRS):
    """One frame {dt [D,H,W], scores [D], gt [G,H,W], crowd [G], ignore [G], gt_area [G] or None (NaN entries: computed), dt_boxes,
    gt_boxes (bbox; None: tight boxes)} -> (iou, dt_area, gt_area as used, [record per area range])."""
    crowd = np.asarray(frame.get("crowd", np.zeros(len(frame["gt"]))), bool)
    ignore = np.asarray(frame.get("ignore", np.zeros(len(frame["gt"]))), bool)
    if iou_type == "segm":
        iou, da, ga = mask_iou_np(frame["dt"], frame["gt"], crowd)
    else:
        db = frame.get("dt_boxes")
        gb = frame.get("gt_boxes")
        iou, da, ga = box_iou_np(tight_boxes_np(frame["dt"]) if db is None else db, tight_boxes_np(frame["gt"]) if gb is None else gb, crowd)
    given = frame.get("gt_area")
    if given is not None:
        given = np.asarray(given, np.float64)
        ga = np.where(np.isnan(given), ga, given)
    recs = [coco_eval_img_np(frame["scores"], da, ga, crowd, ignore, iou, rng, iou_thrs) for rng in area_rng]
    return iou, da, ga, recs


def coco_stats_np(frames, iou_type="segm"):
    """The twelve numbers of a list of frames (coco_frame_np's dicts)."""
    records = [[] for _ in AREA_RNG]
    for fr in frames:
        for a, rec in enumerate(coco_frame_np(fr, iou_type)[3]):
            records[a].append(rec)
    return coco_summarize_np(*coco_accumulate_np(records))


def rect(h, w, y0, x0, hh, ww):
    m = np.zeros((h, w), np.uint8)
    m[y0:y0 + hh, x0:x0 + ww] = 1
    return m


def example_a():
    """Ground truths of 400 and 2000 px; detections .9: 328 px inside the first (IoU .82), .8: 300 px disjoint, .7: 1240 px inside the
    second (IoU .62)."""
    h, w = 64, 128
    gt = np.stack([rect(h, w, 0, 0, 20, 20), rect(h, w, 0, 30, 40, 50)])
    d0 = rect(h, w, 0, 0, 20, 20)
    d0.ravel()[np.flatnonzero(d0)[328:]] = 0
    d1 = rect(h, w, 45, 0, 10, 30)
    d2 = rect(h, w, 0, 30, 40, 31)
    return {"dt": np.stack([d0, d1, d2]), "scores": np.array([.9, .8, .7], np.float32), "gt": gt}


# ---- the hand-derived cases ----
def test_constants():
    assert len(IOU_THRS) == 10 and IOU_THRS[0] == 0.5 and IOU_THRS[5] == 0.75 and IOU_THRS[8] == 0.8999999999999999
    assert len(REC_THRS) == 101 and REC_THRS[0] == 0 and REC_THRS[100] == 1


def test_example_a():
    fr = example_a()
    iou, da, ga, _ = coco_frame_np(fr)
    assert da.tolist() == [328, 300, 1240] and ga.tolist() == [400, 2000]
    assert iou[0, 0] == 328 / 400 and iou[2, 1] == 1240 / 2000 and iou[1].tolist() == [0, 0] and iou[0, 1] == 0 and iou[2, 0] == 0
    stats = coco_stats_np([fr])
    # t <= .60: tp, fp, tp -> precision 1 up to recall .5 (51 recall thresholds), 2/3 up to recall 1 (50); .65 <= t <= .80: only the first
    # detection matches -> 51 thresholds at 1; t >= .85: nothing matches
    ap50, ap75 = (51 + 50 * 2 / 3) / 101, 51 / 101
    want = [(3 * ap50 + 4 * ap75) / 10, ap50, ap75, 0.7, 0.3, -1, 0.35, 0.5, 0.5, 0.7, 0.3, -1]
    np.testing.assert_allclose(stats, want, rtol=0, atol=1e-12)
    assert abs(stats[0] - 0.4524752475247524) < 1e-12


def example_b():
    iou = np.array([[.7, .7, .9], [.6, .2, .9]], np.float64)
    return dict(scores=np.array([.5, .5], np.float32), dt_area=np.array([2000., 2000.]), gt_area=np.array([2000., 2000., 2000.]),
                crowd=np.array([0, 0, 1], bool), ignore=np.zeros(3, bool), iou=iou)


def test_example_b_ties_and_crowd():
    b = example_b()
    rec = coco_eval_img_np(b["scores"], b["dt_area"], b["gt_area"], b["crowd"], b["ignore"], b["iou"], AREA_RNG[0])
    assert rec["order"].tolist() == [0, 1] and rec["gorder"].tolist() == [0, 1, 2] and rec["gtIg"].tolist() == [0, 0, 1]
    # the first detection holds ground truth 1 (the later of the .7 tie) up to t = .70, then the crowd (.9); the second takes ground truth 0
    # (.6) up to t = .60 and is matched to the crowd - and ignored - from t = .65
    want_ig0 = [not .7 >= t for t in IOU_THRS[:9]]
    want_ig1 = [not .6 >= t for t in IOU_THRS[:9]]
    assert want_ig1[:4] == [False, False, False, True] and want_ig0[5:] == [True] * 4
    assert rec["dtm"][:9, 0].all() and rec["dtIg"][:9, 0].tolist() == want_ig0
    assert rec["dtm"][:9, 1].all() and rec["dtIg"][:9, 1].tolist() == want_ig1
    # at t = .95 the crowd's .9 is below the threshold for both: unmatched, inside the area range -> not ignored
    assert not rec["dtm"][9].any() and not rec["dtIg"][9].any()
    # which ground truth: replay t = .5 by hand
    one = coco_eval_img_np(b["scores"][:1], b["dt_area"][:1], b["gt_area"], b["crowd"], b["ignore"], b["iou"][:1], AREA_RNG[0], IOU_THRS[:1])
    assert one["dtm"][0, 0] and not one["dtIg"][0, 0]
    swapped = b["iou"].copy()
    swapped[1, 1] = .6                                   # were the first detection on ground truth 0, the second would take 1 - it cannot
    rec2 = coco_eval_img_np(b["scores"], b["dt_area"], b["gt_area"], b["crowd"], b["ignore"], swapped, AREA_RNG[0], IOU_THRS[:1])
    assert rec2["dtm"][0].tolist() == [True, True] and not rec2["dtIg"][0].any()
    swapped[1] = [.2, .6, 0]                             # the second detection reaches ground truth 1 only: the first one holds it
    rec3 = coco_eval_img_np(b["scores"], b["dt_area"], b["gt_area"], b["crowd"], b["ignore"], swapped, AREA_RNG[0], IOU_THRS[:1])
    assert rec3["dtm"][0].tolist() == [True, False]


def test_perfect_predictions():
    h, w = 120, 160
    gt = np.stack([rect(h, w, 0, 0, 20, 20), rect(h, w, 30, 0, 40, 50), rect(h, w, 0, 60, 100, 100)])     # 400, 2000, 10000 px
    stats = coco_stats_np([{"dt": gt.copy(), "scores": np.array([.9, .8, .7], np.float32), "gt": gt}])
    # (precision is tp / (tp + fp + spacing(1)): one ulp below 1 where tp = 1)
    np.testing.assert_allclose(np.delete(stats, 6), np.ones(11), rtol=0, atol=1e-12)
    assert abs(stats[6] - 1 / 3) < 1e-15                 # one detection per frame reaches one of three ground truths


def test_no_record_without_detections_and_ground_truths():
    e = np.zeros((0, 8, 8), np.uint8)
    recs = coco_frame_np({"dt": e, "scores": np.zeros(0, np.float32), "gt": e})[3]
    assert recs == [None] * 4
    assert coco_stats_np([{"dt": e, "scores": np.zeros(0, np.float32), "gt": e}]).tolist() == [-1] * 12
    # ... and such a frame changes nothing next to another
    fr = example_a()
    assert np.array_equal(coco_stats_np([fr, {"dt": e.reshape(0, 64, 128), "scores": np.zeros(0, np.float32), "gt": e.reshape(0, 64, 128)}]),
                          coco_stats_np([fr]))


def test_area_range_without_ground_truth():
    stats = coco_stats_np([example_a()])
    assert stats[5] == -1 and stats[11] == -1            # no ground truth above 9216 px
    # a frame with ground truths but no detection: recall 0, precision 0 everywhere it is defined
    fr = example_a()
    fr = {"dt": fr["dt"][:0], "scores": fr["scores"][:0], "gt": fr["gt"]}
    assert coco_stats_np([fr]).tolist() == [0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, -1]


def test_box_iou_touching_and_crowd():
    db = np.array([[0., 0., 2.5, 2.], [2.5, 0., 1., 1.]])
    gb = np.array([[0.5, 0.5, 2., 2.], [0., 0., 10., 10.]])
    iou, da, ga = box_iou_np(db, gb, [False, True])
    assert iou[1, 0] == 0.0                              # they touch at x = 2.5: w == 0
    assert iou[0, 0] == (2. * 1.5) / (5. + 4. - 3.) and iou[0, 1] == 1.0 and iou[1, 1] == 1.0
    assert da.tolist() == [5., 1.] and ga.tolist() == [4., 100.]
    assert tight_boxes_np(rect(9, 9, 2, 3, 4, 5)[None]).tolist() == [[3, 2, 5, 4]] and tight_boxes_np(np.zeros((1, 4, 4))).tolist() == [[0, 0, 0, 0]]


def test_package_host_half_equals_contract():
    """accumulate / summarize of quber_amd.eval.coco_ap on the contract's records (no device needed)."""
    from quber_amd.eval import coco_ap
    assert np.array_equal(coco_ap.IOU_THRS, IOU_THRS) and np.array_equal(coco_ap.REC_THRS, REC_THRS)
    assert np.array_equal(coco_ap.AREA_RNG, AREA_RNG) and tuple(coco_ap.MAX_DETS) == MAX_DETS
    rng = np.random.default_rng(5)
    frames = [example_a()]
    for _ in range(3):
        gt = np.stack([rect(48, 64, *rng.integers(0, 20, 2), *rng.integers(4, 28, 2)) for _ in range(4)])
        dt = np.stack([np.roll(g, rng.integers(-3, 4), 1) for g in gt] + [rect(48, 64, 40, 50, 6, 9)])
        frames.append({"dt": dt, "scores": rng.random(5).astype(np.float32), "gt": gt, "crowd": [0, 0, 0, 1]})
    none = {"dt": frames[1]["dt"][:0], "scores": np.zeros(0, np.float32), "gt": frames[1]["gt"]}    # ground truths, no detection
    empty = {"dt": frames[1]["dt"][:0], "scores": np.zeros(0, np.float32), "gt": frames[1]["gt"][:0]}

    def both(frs):
        records = [[] for _ in AREA_RNG]
        for fr in frs:
            for a, rec in enumerate(coco_frame_np(fr)[3]):
                records[a].append(rec)
        p, r = coco_accumulate_np(records)
        gp, gr = coco_ap.accumulate_records(records)
        assert np.array_equal(gp.view(np.uint64), p.view(np.uint64)) and np.array_equal(gr.view(np.uint64), r.view(np.uint64))
        assert np.array_equal(coco_ap.summarize_tables(gp, gr).view(np.uint64), coco_summarize_np(p, r).view(np.uint64))
        return gp, gr

    both(frames)
    both(frames + [none, empty])
    p, r = both([none, none])                            # no detection at all: recall 0 and precision 0 where a ground truth counts
    assert (r[:, 0] == 0).all() and (p[:, :, 0] == 0).all() and (r[:, 3] == -1).all()
    p, r = both([empty])
    assert (p == -1).all() and (r == -1).all()
