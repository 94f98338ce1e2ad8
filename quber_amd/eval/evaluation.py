"""Drop-in for the reference's ``eval/evaluation.py:multilabel_metrics`` (lines 57-274): Objects P / R / F, their
object-size-normalised variants, F@.75 detection counts, the IoU measures and the Boundary P / R / F.  All pairwise overlap
counts come from ONE pass of a HIP kernel over the two label maps instead of one numpy pass per pair; the boundary
true-positive counts of every pair (evaluation.py:21-54) come from three launches on bit planes (csrc/boundary.hip:
seg2bmap as an outside flood fill + 4-neighbour test, disk dilation as shifted ORs).

``multilabel_metrics_batch`` (``enqueue_metrics`` + ``collect_metrics``) evaluates B pairs in one call (csrc/evalbatch.hip): the tables, the
F-measure matrix and the Munkres assignment stay on the device, one copy comes back, and ``_metrics_from_tables`` - the final arithmetic
both paths share - turns every frame's record into the dictionary the per-frame function returns, bit for bit.

The overlap half reproduces the imported reference bit for bit (tests/golden/metrics_*.npz).  The boundary half restates
cv2.findContours / drawContours / dilate and skimage's disk from their published algorithms (neither library is in the
image): parity unpinned."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .assignment import munkres_assign

BACKGROUND_LABEL = 0
CAP = 256


def contingency(prediction, gt, device="cuda:0"):
    """-> (labels_pred, labels_gt, table[n_gt, n_pred]) with np.unique ordering; integer label maps of equal shape."""
    lib = _lib.load()
    prediction, gt = np.asarray(prediction), np.asarray(gt)
    assert prediction.shape == gt.shape
    remap = None
    lo = min(int(prediction.min()), int(gt.min())) if prediction.size else 0
    hi = max(int(prediction.max()), int(gt.max())) if prediction.size else 0
    if lo < 0 or hi > 65535:
        # the reference's np.unique accepts any integers (e.g. the -1 void label of panoptic_seg, or label * 1000 ids); the
        # kernel's LUT covers 0..65535, so such maps are renumbered densely first (order-preserving, mapped back below)
        vals = np.unique(np.concatenate([np.unique(prediction), np.unique(gt)]))
        if vals.size > 65536:
            raise ValueError("more than 65536 distinct labels")
        prediction, gt, remap = np.searchsorted(vals, prediction), np.searchsorted(vals, gt), vals
    p = torch.as_tensor(np.ascontiguousarray(prediction)).to(device=device, dtype=torch.int32).contiguous()
    g = torch.as_tensor(np.ascontiguousarray(gt)).to(device=device, dtype=torch.int32).contiguous()
    nbytes = lib.quber_contingency_workspace_bytes(CAP)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _lib.check(lib.quber_label_contingency(C.c_void_p(p.data_ptr()), C.c_void_p(g.data_ptr()), p.numel(), CAP,
                                           C.c_void_p(ws.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    o = 2 * 65536 * 4
    host = ws[o:o + CAP * CAP * 8 + 2 * CAP * 4 + 16].cpu().numpy()
    table = host[:CAP * CAP * 8].view(np.uint64).reshape(CAP, CAP)
    labels = host[CAP * CAP * 8:CAP * CAP * 8 + 2 * CAP * 4].view(np.int32).reshape(2, CAP)
    n_pred, n_gt, bad, _ = host[CAP * CAP * 8 + 2 * CAP * 4:].view(np.int32)
    if bad:
        raise ValueError("label values must lie in 0..65535")
    if n_pred > CAP or n_gt > CAP:
        raise ValueError(f"more than {CAP} distinct labels in a map")
    lp, lg = labels[0, :n_pred].astype(np.int64), labels[1, :n_gt].astype(np.int64)
    if remap is not None:
        lp, lg = remap[lp].astype(np.int64), remap[lg].astype(np.int64)
    return lp, lg, table[:n_gt, :n_pred].astype(np.int64)


def _degenerate(p, r, f, num_pred, num_gt, pct):
    return {'Objects F-measure': f, 'Objects Precision': p, 'Objects Recall': r,
            'Boundary F-measure': f, 'Boundary Precision': p, 'Boundary Recall': r,
            'Objects OSN F-measure': f, 'Objects OSN Precision': p, 'Objects OSN Recall': r,
            'Boundary OSN F-measure': f, 'Boundary OSN Precision': p, 'Boundary OSN Recall': r,
            'obj_detected': num_pred, 'obj_detected_075': 0., 'obj_gt': num_gt,
            'obj_detected_075_percentage': pct, 'obj_detected_075_percentage_normalized': pct}


def boundary_counts(prediction, gt, labels_pred, labels_gt, bound_th=0.003, device="cuda:0"):
    """-> (bound_counts_pred [n_pred], bound_counts_gt [n_gt], precision_tps [n_gt, n_pred], recall_tps [n_gt, n_pred]) as
    float64, for the given object labels (evaluation.py:165-175 and :21-54 for every pair)."""
    lib = _lib.load()
    prediction, gt = np.asarray(prediction), np.asarray(gt)
    h, w = prediction.shape
    n_pred, n_gt = len(labels_pred), len(labels_gt)
    bound_pix = int(bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm(prediction.shape)))
    p = torch.as_tensor(np.ascontiguousarray(prediction)).to(device=device, dtype=torch.int32).contiguous()
    g = torch.as_tensor(np.ascontiguousarray(gt)).to(device=device, dtype=torch.int32).contiguous()
    labels = torch.as_tensor(np.concatenate([labels_pred, labels_gt]).astype(np.int32)).to(device)
    ws = torch.empty(lib.quber_boundary_workspace_bytes(h, w, n_pred + n_gt), dtype=torch.uint8, device=device)
    out = torch.empty(n_pred + n_gt + 2 * n_pred * n_gt, dtype=torch.int32, device=device)
    _lib.check(lib.quber_boundary_overlap(C.c_void_p(p.data_ptr()), C.c_void_p(g.data_ptr()), h, w, C.c_void_p(labels.data_ptr()),
                                          n_pred, n_gt, bound_pix, C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    o = out.cpu().numpy().astype(np.float64)
    nm = n_pred + n_gt
    return (o[:n_pred], o[n_pred:nm], o[nm:nm + n_gt * n_pred].reshape(n_gt, n_pred),
            o[nm + n_gt * n_pred:].reshape(n_gt, n_pred))


def _metrics_from_tables(lp, lg, table, assignments=None, boundary=None, obj_detect_threshold=0.75):
    """The final arithmetic of multilabel_metrics (evaluation.py:104-274), shared by the per-frame and the batched path.
    lp / lg: sorted unique labels of the prediction / the ground truth; table int64 [len(lg), len(lp)]: the contingency table;
    assignments: [(gt object, predicted object)] of the Munkres step, or None: solved here; boundary: None, the tuple
    (bc_pred, bc_gt, ptps, rtps) of boundary_counts, or a callable (labels_pred, labels_gt) -> that tuple, called only for a frame
    that has objects on both sides.  Every float sum stays a numpy sum in the reference's order."""
    area_pred, area_gt = table.sum(axis=0), table.sum(axis=1)     # incl. the background row / column
    kp, kg = lp != BACKGROUND_LABEL, lg != BACKGROUND_LABEL
    num_pred, num_gt = int(kp.sum()), int(kg.sum())
    # edge cases of evaluation.py:104-162
    if num_pred == 0 and num_gt > 0:
        return _degenerate(1., 0., 0., num_pred, num_gt, 0.)
    if num_pred > 0 and num_gt == 0:
        return _degenerate(0., 1., 0., num_pred, num_gt, 0.)
    if num_pred == 0 and num_gt == 0:
        return _degenerate(1., 1., 1., num_pred, num_gt, 1.)
    tps = table[np.ix_(kg, kp)].astype(np.float64)                # obj_tps[i, j] = |gt_i & pred_j|
    ap, ag = area_pred[kp].astype(np.float64), area_gt[kg].astype(np.float64)
    union = ag[:, None] + ap[None, :] - tps
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = tps / union
        P, R = tps / ap[None, :], tps / ag[:, None]
        F = (2 * P * R) / (P + R)
    F[np.isnan(F)] = 0
    if assignments is None:
        assignments = munkres_assign(F.max() - F)
    assignments = [(int(i), int(j)) for i, j in assignments]
    idx = tuple(np.array(assignments).T)
    detected = sum(1 for a in assignments if F[a] > obj_detect_threshold)
    fg_pred = float(area_pred[lp >= 1].sum())                      # np.sum(prediction.clip(0,1) == 1)
    fg_gt = float(area_gt[lg >= 1].sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = np.sum(tps[idx]) / fg_pred
        recall = np.sum(tps[idx]) / fg_gt
        f_measure = (2 * precision * recall) / (precision + recall)
        if np.isnan(f_measure):
            f_measure = 0
        b = dict.fromkeys(("F", "P", "R", "Fo", "Po", "Ro"))
        if boundary is not None:                                     # evaluation.py:165-175, 200-206, 232-243
            bc_pred, bc_gt, ptps, rtps = boundary(lp[kp], lg[kg]) if callable(boundary) else boundary
            bP, bR = ptps / bc_pred[None, :], rtps / bc_gt[:, None]
            bF = (2 * bP * bR) / (bP + bR)
            bF[np.isnan(bF)] = 0
            b["P"], b["R"] = np.sum(ptps[idx]) / np.sum(bc_pred), np.sum(rtps[idx]) / np.sum(bc_gt)
            b["F"] = (2 * b["P"] * b["R"]) / (b["P"] + b["R"])
            if np.isnan(b["F"]):
                b["F"] = 0
            b["Fo"], b["Po"], b["Ro"] = np.sum(bF[idx]) / max(num_pred, num_gt), np.sum(bP[idx]) / num_pred, np.sum(bR[idx]) / num_gt
        out = {'Objects F-measure': f_measure, 'Objects Precision': precision, 'Objects Recall': recall,
               'Boundary F-measure': b["F"], 'Boundary Precision': b["P"], 'Boundary Recall': b["R"],
               'Objects OSN F-measure': np.sum(F[idx]) / max(num_pred, num_gt),
               'Objects OSN Precision': np.sum(P[idx]) / num_pred, 'Objects OSN Recall': np.sum(R[idx]) / num_gt,
               'Boundary OSN F-measure': b["Fo"], 'Boundary OSN Precision': b["Po"], 'Boundary OSN Recall': b["Ro"],
               'obj_detected': num_pred, 'obj_detected_075': detected, 'obj_gt': num_gt,
               'obj_detected_075_percentage': detected / num_gt,
               'obj_detected_075_percentage_normalized': detected / max(num_gt, num_pred),
               'obj_mIOU_osn': np.mean(iou[idx]), 'obj_mIOU': np.sum(tps[idx]) / np.sum(union[idx])}
    return out


def multilabel_metrics(prediction, gt, i=0, N=0, obj_detect_threshold=0.75, compute_boundary_stuff=True, verbose=False,
                       device="cuda:0"):
    lp, lg, table = contingency(prediction, gt, device)
    boundary = (lambda op, og: boundary_counts(prediction, gt, op, og, device=device)) if compute_boundary_stuff else None
    return _metrics_from_tables(lp, lg, table, None, boundary, obj_detect_threshold)


# ------------------------------------------------------------------------------------------------ the batched path (csrc/evalbatch.hip)
_EVAL_WS = {}           # (device, stream, B, h, w, cap, with_boundary) -> workspace tensor; the calls of one stream are ordered, so its handles share it
_EVAL_WS_MAX = 8
STATUS_BAD_LABEL, STATUS_OVER_CAP, STATUS_SOLVER_BOUND, STATUS_NO_LDS = 1, 2, 4, 8


def record_layout(cap):
    """Byte offsets of one frame's record in quber_eval_batch's dev_out (include/quber_hip.h) -> (offsets dict, record bytes)."""
    c, cc = cap, cap * cap
    off, o = {}, 0
    for name, nbytes in (("table", 8 * cc), ("F", 8 * cc), ("area", 16 * c), ("pair_tps", 8 * c), ("pair_union", 8 * c),
                         ("ptps", 4 * cc), ("rtps", 4 * cc), ("hdr", 32), ("labels", 8 * c), ("bc", 8 * c), ("assign", 4 * c),
                         ("pairs", 8 * c), ("pair_ptps", 4 * c), ("pair_rtps", 4 * c)):
        off[name] = o
        o += nbytes
    return off, (o + 7) & ~7


class MetricsList(list):
    """The dicts of collect_metrics.  `fallback`: {frame index: status} of the frames the batched call flagged (quber_eval_batch's
    status bits) and the per-frame multilabel_metrics answered instead; `tables`: per frame the stage tables (return_tables=True)."""
    fallback = None
    tables = None


class _Handle:
    pass


def _workspace(lib, device, B, h, w, cap, with_boundary):
    key = (str(device), torch.cuda.current_stream().cuda_stream, B, h, w, cap, with_boundary)
    ws = _EVAL_WS.get(key)
    if ws is None:
        if len(_EVAL_WS) >= _EVAL_WS_MAX:
            _EVAL_WS.pop(next(iter(_EVAL_WS)))
        nbytes = lib.quber_eval_batch_workspace_bytes(B, h, w, cap, with_boundary)
        if nbytes <= 0:
            raise ValueError(f"batched metrics: no workspace for batch {B}, {h} x {w}, cap {cap}")
        ws = _EVAL_WS[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def _as_device_maps(a, device):
    """-> (int32 device tensor [B,H,W], the numpy original or None)."""
    if isinstance(a, torch.Tensor):
        if not a.is_cuda or a.dtype != torch.int32 or a.dim() != 3:
            raise ValueError("batched metrics: tensors must be int32 [B,H,W] on the device (numpy arrays: any integer type)")
        return a.contiguous(), None
    host = np.asarray(a)
    if host.ndim != 3 or host.dtype.kind not in "iub":
        raise ValueError("batched metrics: label maps must be integer arrays [B,H,W]")
    narrow = host
    if host.dtype.itemsize > 4 or host.dtype == np.uint32:
        narrow = np.clip(host, -1, 65536)        # what int32 cannot hold stays outside 0..65535: the frame is flagged, never aliased
    return torch.from_numpy(np.ascontiguousarray(narrow, dtype=np.int32)).to(device), host


def enqueue_metrics(preds, gts, compute_boundary_stuff=True, cap=64, bound_th=0.003, placement=0, obj_detect_threshold=0.75,
                    return_tables=False, device="cuda:0"):
    """multilabel_metrics for B pairs of label maps, enqueued on the current stream with nothing read back -> handle for collect_metrics.
    preds, gts: numpy integer arrays or device int32 tensors [B,H,W].  cap: most distinct labels per map (background included) the
    batched call handles, 1..256; placement: where the solver keeps its cost matrix (0 auto, 1 LDS, 2 device memory)."""
    lib = _lib.load()
    p, p_host = _as_device_maps(preds, device)
    g, g_host = _as_device_maps(gts, p.device if isinstance(preds, torch.Tensor) else device)
    if p.shape != g.shape or p.device != g.device:
        raise ValueError("batched metrics: predictions and ground truths differ in shape or device")
    B, h, w = (int(v) for v in p.shape)
    with_boundary = int(bool(compute_boundary_stuff))
    bound_pix = int(bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm((h, w))))
    hd = _Handle()
    hd.shape, hd.cap, hd.with_boundary, hd.threshold, hd.return_tables = (B, h, w), int(cap), with_boundary, obj_detect_threshold, return_tables
    hd.device = p.device
    hd.inputs = (p, g)                       # alive until collected
    hd.host = (p_host, g_host)
    hd.offsets, hd.record = record_layout(hd.cap)
    if B == 0:
        hd.out = None
        return hd
    with torch.cuda.device(p.device):
        ws = _workspace(lib, p.device, B, h, w, hd.cap, with_boundary)
        hd.out = torch.empty(B * hd.record, dtype=torch.uint8, device=p.device)
        _lib.check(lib.quber_eval_batch(C.c_void_p(p.data_ptr()), C.c_void_p(g.data_ptr()), B, h, w, hd.cap, bound_pix, with_boundary,
                                        int(placement), C.c_void_p(ws.data_ptr()), C.c_void_p(hd.out.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        hd.done = torch.cuda.Event()
        hd.done.record()
    return hd


def collect_metrics(handle):
    """-> MetricsList of the dicts multilabel_metrics returns, one per pair, after ONE device-to-host copy."""
    hd = handle
    res = MetricsList()
    res.fallback = {}
    res.tables = [] if hd.return_tables else None
    B, h, w = hd.shape
    if B == 0:
        return res
    hd.done.synchronize()
    host = hd.out.cpu().numpy().reshape(B, hd.record)
    cap, off = hd.cap, hd.offsets

    def field(b, name, dtype, count):
        return host[b, off[name]:off[name] + count * np.dtype(dtype).itemsize].view(dtype)

    for b in range(B):
        n_pred, n_gt, _, status, no_p, no_g, n_pairs, _ = (int(v) for v in field(b, "hdr", np.int32, 8))
        if status:
            if status & STATUS_BAD_LABEL and hd.host[0] is None and hd.host[1] is None:
                raise ValueError(f"batched metrics: frame {b} has label values outside 0..65535")
            # flagged: answered by the per-frame function (which renumbers out-of-range labels of numpy input, as contingency does)
            pm = hd.host[0][b] if hd.host[0] is not None else hd.inputs[0][b].cpu().numpy()
            gm = hd.host[1][b] if hd.host[1] is not None else hd.inputs[1][b].cpu().numpy()
            res.append(multilabel_metrics(pm, gm, obj_detect_threshold=hd.threshold, compute_boundary_stuff=bool(hd.with_boundary),
                                          device=hd.device))
            res.fallback[b] = status
            if hd.return_tables:
                res.tables.append({"status": status, "fallback": True})
            continue
        labels = field(b, "labels", np.int32, 2 * cap).reshape(2, cap)
        lp, lg = labels[0, :n_pred].astype(np.int64), labels[1, :n_gt].astype(np.int64)
        table = field(b, "table", np.uint64, cap * cap).reshape(cap, cap)[:n_gt, :n_pred].astype(np.int64)
        pairs = field(b, "pairs", np.int32, 2 * cap).reshape(cap, 2)[:n_pairs]
        assignment = [(int(i), int(j)) for i, j in pairs]
        boundary = None
        if hd.with_boundary:
            bc = field(b, "bc", np.uint32, 2 * cap).reshape(2, cap).astype(np.float64)
            ptps = field(b, "ptps", np.uint32, cap * cap).reshape(cap, cap)[:no_g, :no_p].astype(np.float64)
            rtps = field(b, "rtps", np.uint32, cap * cap).reshape(cap, cap)[:no_g, :no_p].astype(np.float64)
            boundary = (bc[0, :no_p], bc[1, :no_g], ptps, rtps)
        res.append(_metrics_from_tables(lp, lg, table, assignment, boundary, hd.threshold))
        if hd.return_tables:
            t = {"labels_pred": lp, "labels_gt": lg, "table": table, "status": status, "fallback": False, "assignment": assignment,
                 "F": field(b, "F", np.float64, cap * cap).reshape(cap, cap)[:no_g, :no_p].copy(),
                 "bc_pred": None, "bc_gt": None, "ptps": None, "rtps": None,
                 "pair_tps": field(b, "pair_tps", np.uint64, cap)[:n_pairs].astype(np.int64),
                 "pair_union": field(b, "pair_union", np.uint64, cap)[:n_pairs].astype(np.int64),
                 "pair_ptps": field(b, "pair_ptps", np.uint32, cap)[:n_pairs].astype(np.int64),
                 "pair_rtps": field(b, "pair_rtps", np.uint32, cap)[:n_pairs].astype(np.int64)}
            if boundary is not None:
                t["bc_pred"], t["bc_gt"], t["ptps"], t["rtps"] = boundary
            res.tables.append(t)
    return res


def multilabel_metrics_batch(preds, gts, compute_boundary_stuff=True, cap=64, bound_th=0.003, placement=0, obj_detect_threshold=0.75,
                             return_tables=False, device="cuda:0"):
    """[multilabel_metrics(p, g) for p, g in zip(preds, gts)], bit for bit, from one enqueue and one copy back.  With
    return_tables=True -> (dicts, tables)."""
    res = collect_metrics(enqueue_metrics(preds, gts, compute_boundary_stuff, cap, bound_th, placement, obj_detect_threshold,
                                          return_tables, device))
    return (res, res.tables) if return_tables else res
