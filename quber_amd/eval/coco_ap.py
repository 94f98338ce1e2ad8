"""COCO mask / box AP and AR of scored instance masks, for one class-agnostic category: what the reference prints after every evaluation
period through detectron2's COCOEvaluator(use_fast_impl=False) and pycocotools (train_net.py:57, maskrefiner/evaluation/
instance_evaluation.py).  The per-frame half - pairwise IoU, the top 100 by score, the greedy matching per threshold and area range - runs
on the device (csrc/cocoap.hip: quber_coco_match), one small record per frame comes back; accumulate and summarize run here on those
records.  The definition is tests/test_cocoap_cpu.py (numpy in plain loops) and DESIGN.md "COCO AP"; parity with pycocotools is unpinned.
iou_type "boundary" is Boundary AP (Cheng et al.; the reference's tools/evaluate_coco_boundary_ap.py): the same with iou = min(mask IoU,
Boundary IoU), the boundaries made on the device (csrc/boundaryap.hip: quber_coco_match_boundary); tests/test_boundary_ap_cpu.py and
DESIGN.md "Boundary AP" hold the definition, parity with the boundary_iou package is argued, not pinned."""
import math
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..engine import Engine, _ptr, _stream, make_config

# the constants of COCOeval's Params, built the way it builds them; handed to the device as these float64 bits
IOU_THRS = np.linspace(.5, .95, int(np.round((.95 - .5) / .05)) + 1)
REC_THRS = np.linspace(0, 1, 101)
AREA_RNG = np.array([[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]], np.float64)
MAX_DETS = (1, 10, 100)
TOP = 100                          # csrc/cocoap.hip: CA_TOP
MAX_N = 1024                       # ... CA_MAX: detections / ground truths per frame
ABSENT = 0xFF                      # gt_flags of a padding slot; bit 0 = crowd, bit 1 = ignore
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
MAX_BATCH = 16                     # frames per call of an engine; a larger batch goes in pieces
MAX_LABELS = 254                   # labels per frame of a label-map ground truth (quber_config.top_k's maximum)
MAX_DILATION = 64                  # csrc/boundaryap.hip: CB_MAX_D


def boundary_dilation(h, w, ratio=0.02):
    """The dilation distance of Boundary IoU for an h x w frame (boundary-iou-api's mask_to_boundary): ratio x the diagonal, rounded with
    Python's round, at least 1.  480 x 640 -> 16."""
    return max(1, int(round(ratio * math.sqrt(h * h + w * w))))


def accumulate_records(records, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS):
    """COCOeval.accumulate.  records[a]: the frame records {scores f32 [nd], dtm, dtIg bool [T,nd], gtIg [n_gt]} of area range a (None: a
    frame without detections and ground truths) -> (precision [T,R,A,M], recall [T,A,M]), -1 where nothing can be said."""
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(records), len(max_dets)
    precision, recall = np.full((T, R, A, M), -1.0), np.full((T, A, M), -1.0)
    for a in range(A):
        E = [e for e in records[a] if e is not None]
        if not E:
            continue
        npig = sum(int(np.count_nonzero(np.asarray(e["gtIg"]) == 0)) for e in E)
        if npig == 0:
            continue
        for mi, md in enumerate(max_dets):
            scores = np.concatenate([e["scores"][:md] for e in E])
            inds = np.argsort(-scores, kind="mergesort")
            dtm = np.concatenate([np.asarray(e["dtm"], bool)[:, :md] for e in E], axis=1)[:, inds]
            dtig = np.concatenate([np.asarray(e["dtIg"], bool)[:, :md] for e in E], axis=1)[:, inds]
            tp = np.cumsum(dtm & ~dtig, axis=1).astype(float)
            fp = np.cumsum(~dtm & ~dtig, axis=1).astype(float)
            nd = tp.shape[1]
            if nd == 0:
                recall[:, a, mi], precision[:, :, a, mi] = 0.0, 0.0
                continue
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            recall[:, a, mi] = rc[:, -1]
            pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]         # non-increasing from the right
            for t in range(T):
                ix = np.searchsorted(rc[t], rec_thrs, side="left")
                precision[t, :, a, mi] = np.where(ix < nd, pr[t][np.minimum(ix, nd - 1)], 0.0)
    return precision, recall


def summarize_tables(precision, recall):
    """COCOeval.summarize -> the twelve numbers of STAT_NAMES (-1: undefined)."""
    def mean(x):
        x = x[x > -1]
        return float(np.mean(x)) if x.size else -1.0
    m = precision.shape[3] - 1
    ap = [precision[:, :, 0, m], precision[0, :, 0, m], precision[5, :, 0, m], precision[:, :, 1, m], precision[:, :, 2, m], precision[:, :, 3, m]]
    ar = [recall[:, 0, 0], recall[:, 0, 1], recall[:, 0, 2], recall[:, 1, m], recall[:, 2, m], recall[:, 3, m]]
    return np.array([mean(x) for x in ap + ar], np.float64)


_ENGINES = {}


def _engine(h, w, device):
    key = (h, w, str(device))
    if key not in _ENGINES:
        qc = make_config(h, w, max_batch=MAX_BATCH, with_network=False)
        qc.top_k = MAX_LABELS                  # the table of quber_extract_masks: as many labels as compact_labels allows
        _ENGINES[key] = Engine(qc, device)
    return _ENGINES[key]


def close_engines():
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


class _Handle:
    __slots__ = ("buf", "views", "B", "n_gt", "event")


class CocoAP:
    """iou_type "segm", "bbox" or "boundary".  update() / enqueue() + collect() per batch, then summarize() -> stats (12 floats), results()
    -> the dict detectron2 reports.  One category; RLE / polygon inputs, COCO json and per-category tables are out of scope.
    "boundary": iou = min(mask IoU, Boundary IoU) with the dilation distance boundary_dilation(H, W, dilation_ratio) of every call's frame,
    or `dilation` (1..64 pixels) where that is given; inputs and outputs are those of "segm"."""

    def __init__(self, iou_type="segm", device="cuda:0", dilation_ratio=0.02, dilation=None):
        if iou_type not in ("segm", "bbox", "boundary"):
            raise ValueError(f"iou_type={iou_type!r}: expected 'segm', 'bbox' or 'boundary'")
        if not (isinstance(dilation_ratio, (int, float)) and 0 < dilation_ratio < math.inf):
            raise ValueError(f"dilation_ratio={dilation_ratio!r}: expected a positive number")
        if dilation is not None and (isinstance(dilation, bool) or not isinstance(dilation, (int, np.integer)) or not 1 <= dilation <= MAX_DILATION):
            raise ValueError(f"dilation={dilation!r}: expected an integer in 1..{MAX_DILATION}")
        if not torch.cuda.is_available():
            raise _lib.QuberError("CocoAP needs a ROCm GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.iou_type, self.device = iou_type, torch.device(device)
        self.dilation_ratio, self.dilation = float(dilation_ratio), None if dilation is None else int(dilation)
        self._thrs = torch.from_numpy(IOU_THRS).to(self.device)
        self._rng = torch.from_numpy(AREA_RNG).to(self.device)
        self.reset()

    def reset(self):
        self.records = [[] for _ in AREA_RNG]
        self.frames = 0
        self._tables = None

    # ---- inputs ----
    def _dev(self, x, dtype=None):
        if x is None:
            return None
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if x.dtype == torch.bool:
            x = x.view(torch.uint8) if x.is_contiguous() else x.to(torch.uint8)
        elif dtype is None and x.dtype != torch.uint8:   # masks of another dtype: non-zero = inside
            x = (x != 0).view(torch.uint8)
        if dtype is not None and x.dtype != dtype:
            x = x.to(dtype)
        return x.to(self.device).contiguous()

    def _expand_labels(self, labels):
        """Label maps int [B,H,W] -> (masks u8 [B,n,H,W], flags u8 [B,n]): one mask per non-zero label in ascending order, through
        quber_extract_masks (the label map as its float32 panoptic map, the labels as its table).  The labels of every frame are found
        on the host (np.unique): a label map that lives on the device is copied back first, so this path synchronises."""
        host = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
        if host.dtype.kind not in "iu":
            raise ValueError(f"CocoAP: a label map [B,H,W] must be of an integer dtype, not {host.dtype}")
        B, h, w = host.shape
        eng = _engine(h, w, self.device)
        values = [np.unique(m) for m in host]
        values = [v[v != 0] for v in values]
        n = max((len(v) for v in values), default=0)
        if any((v < 0).any() or (v >= 1 << 24).any() for v in values) or n > eng.cap:
            raise ValueError(f"gt label map: labels must lie in 1..2^24 - 1 and a frame may hold at most {eng.cap}; pass masks instead")
        flags = np.full((B, n), ABSENT, np.uint8)
        table = np.full((B, eng.cap), -1.0, np.float32)
        for b, v in enumerate(values):
            flags[b, :len(v)], table[b, :len(v)] = 0, v
        if n == 0:
            return torch.empty((B, 0, h, w), dtype=torch.uint8, device=self.device), flags
        pan, tab = self._dev(host.astype(np.float32), torch.float32), self._dev(table, torch.float32)
        out = torch.empty((B, n, h, w), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            for b0 in range(0, B, MAX_BATCH):
                b1 = min(B, b0 + MAX_BATCH)
                eng.extract_masks({"panoptic": pan[b0:b1], "labels": tab[b0:b1]}, n, out[b0:b1])
        return out, flags

    def enqueue(self, dt_masks, dt_scores, gt_masks, gt_flags=None, gt_areas=None, dt_boxes=None, gt_boxes=None, buf=None):
        """dt_masks [B,n_dt,H,W] (non-zero = inside), dt_scores [B,n_dt] (NaN: no such detection), gt_masks [B,n_gt,H,W] or an int label
        map [B,H,W] (told apart by the number of axes; a label map's labels are found on the host, so that form synchronises, and a
        frame may hold at most 254); gt_flags u8 [B,n_gt] (bit 0 crowd, bit 1 ignore, 0xFF: no such ground truth; default 0), gt_areas f64 [B,n_gt] (NaN:
        the computed area); bbox mode: dt_boxes [B,n_dt,4], gt_boxes [B,n_gt,4] as x, y, w, h (default: the tight box of each mask; a side whose boxes are given may pass None for its masks).
        torch device tensors or numpy; one frame may come without the leading axis.  With masks the call only launches.  buf: a uint8 device tensor to write the records into
        (default: a fresh one per call).  Asynchronous -> a handle for collect()."""
        one = (dt_scores.dim() if isinstance(dt_scores, torch.Tensor) else np.ndim(dt_scores)) == 1
        lead = (lambda x: x if x is None or not one else x[None])
        scores = self._dev(lead(dt_scores), torch.float32)
        db, gb = self._dev(lead(dt_boxes), torch.float64), self._dev(lead(gt_boxes), torch.float64)
        if self.iou_type != "bbox" and (db is not None or gb is not None):
            raise ValueError("CocoAP: boxes come with iou_type='bbox'")
        if (dt_masks is None and db is None) or (gt_masks is None and gb is None):
            raise ValueError("CocoAP: masks may be None only in bbox mode, on a side whose boxes are given")
        if scores.dim() != 2:
            raise ValueError("CocoAP: dt_scores [B,n_dt], or [n_dt] for one frame")
        B, n_dt = scores.shape
        gt = None
        if gt_masks is not None:
            gt_masks = lead(gt_masks if isinstance(gt_masks, torch.Tensor) else np.asarray(gt_masks))
            if gt_masks.ndim == 3:                       # [B,H,W]: a label map of any integer dtype, uint8 included
                if gt_flags is not None:
                    raise ValueError("CocoAP: gt_flags come with gt masks [B,n_gt,H,W], not with a label map [B,H,W]")
                gt, gt_flags = self._expand_labels(gt_masks)
            elif gt_masks.ndim == 4:
                gt, gt_flags = self._dev(gt_masks), lead(gt_flags)
            else:
                raise ValueError(f"CocoAP: ground truth of shape {tuple(gt_masks.shape)}: expected masks [B,n_gt,H,W] or a label map [B,H,W] "
                                 "(one frame: [n_gt,H,W] or [H,W], with scores [n_dt])")
        else:
            gt_flags = lead(gt_flags)
        dt = self._dev(lead(dt_masks))
        n_gt = gt.shape[1] if gt is not None else gb.shape[1]
        sizes = {tuple(m.shape[2:]) for m in (dt, gt) if m is not None and m.dim() == 4}
        if len(sizes) > 1 or any(m is not None and (m.dim() != 4 or tuple(m.shape[:2]) != (B, n)) for m, n in ((dt, n_dt), (gt, n_gt))):
            raise ValueError(f"CocoAP: detections {None if dt is None else tuple(dt.shape)}, scores {tuple(scores.shape)} and ground truths "
                             f"{None if gt is None else tuple(gt.shape)} do not agree")
        h, w = sizes.pop() if sizes else (16, 16)        # boxes only: the frame size plays no part
        if n_dt > MAX_N or n_gt > MAX_N:
            raise ValueError(f"CocoAP: at most {MAX_N} detections and {MAX_N} ground truths per frame")
        flags = self._dev(np.zeros((B, n_gt), np.uint8) if gt_flags is None else gt_flags, torch.uint8)
        areas = self._dev(lead(gt_areas), torch.float64)
        for name, t, shape in (("gt_flags", flags, (B, n_gt)), ("gt_areas", areas, (B, n_gt)), ("dt_boxes", db, (B, n_dt, 4)), ("gt_boxes", gb, (B, n_gt, 4))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f"CocoAP: {name} of shape {tuple(t.shape)}, expected {shape}")
        T, A = len(IOU_THRS), len(AREA_RNG)
        boundary = self.iou_type == "boundary"
        if boundary:
            d = self.dilation if self.dilation is not None else boundary_dilation(h, w, self.dilation_ratio)
            if d > MAX_DILATION:
                raise ValueError(f"CocoAP: a dilation distance of {d} pixels for a {h} x {w} frame; at most {MAX_DILATION} (pass dilation=)")
        # one buffer for the B records: sections with the frame axis first, the widest elements first (every section stays aligned)
        both = (("mask_iou", np.float64, (TOP, n_gt)), ("boundary_iou", np.float64, (TOP, n_gt))) if boundary else ()
        sections = (("iou", np.float64, (TOP, n_gt)),) + both + (("dt_area", np.float64, (TOP,)), ("gt_area", np.float64, (n_gt,)),
                    ("counts", np.int32, (2,)), ("order", np.int32, (TOP,)), ("gorder", np.int32, (A, n_gt)), ("scores", np.float32, (TOP,)),
                    ("dtm", np.uint8, (A, T, TOP)), ("dtIg", np.uint8, (A, T, TOP)), ("gi", np.uint8, (A, n_gt)))
        offs, total = {}, 0
        for name, dtype, shape in sections:
            offs[name] = (total, np.dtype(dtype), (B,) + shape)
            total += (B * int(np.prod(shape)) * np.dtype(dtype).itemsize + 7) // 8 * 8
        hd = _Handle()
        if buf is None:
            buf = torch.empty((max(total, 8),), dtype=torch.uint8, device=self.device)
        if buf.dtype != torch.uint8 or not buf.is_cuda or buf.dim() != 1 or buf.numel() < total or buf.data_ptr() % 8:
            raise ValueError(f"CocoAP: buf must be an 8-byte aligned uint8 device tensor of at least {total} bytes")
        hd.buf = buf[:max(total, 8)]
        hd.views, hd.B, hd.n_gt = offs, B, n_gt
        eng = _engine(h, w, self.device)
        base = hd.buf.data_ptr()

        def out(name, b0):
            o, dtype, shape = offs[name]
            return C.c_void_p(base + o + b0 * int(np.prod(shape[1:])) * dtype.itemsize)

        def part(t, b0, b1):
            return _ptr(t[b0:b1]) if t is not None and t[b0:b1].numel() else C.c_void_p(0)

        with torch.cuda.device(self.device):
            for b0 in range(0, B, MAX_BATCH):
                b1 = min(B, b0 + MAX_BATCH)
                if boundary:
                    _lib.check(eng.lib.quber_coco_match_boundary(
                        eng.h, part(dt, b0, b1), part(scores, b0, b1), n_dt, part(gt, b0, b1), part(flags, b0, b1), part(areas, b0, b1), n_gt,
                        b1 - b0, d, _ptr(self._thrs), T, _ptr(self._rng), A, out("counts", b0), out("order", b0), out("scores", b0),
                        out("dt_area", b0), out("gt_area", b0), out("iou", b0), out("mask_iou", b0), out("boundary_iou", b0), out("dtm", b0),
                        out("dtIg", b0), out("gi", b0), out("gorder", b0), _stream()))
                    continue
                _lib.check(eng.lib.quber_coco_match(
                    eng.h, part(dt, b0, b1), part(scores, b0, b1), part(db, b0, b1), n_dt, part(gt, b0, b1), part(flags, b0, b1),
                    part(areas, b0, b1), part(gb, b0, b1), n_gt, b1 - b0, 0 if self.iou_type == "segm" else 1, _ptr(self._thrs), T,
                    _ptr(self._rng), A, out("counts", b0), out("order", b0), out("scores", b0), out("dt_area", b0), out("gt_area", b0),
                    out("iou", b0), out("dtm", b0), out("dtIg", b0), out("gi", b0), out("gorder", b0), _stream()))
            hd.event = torch.cuda.Event()
            hd.event.record()
        return hd

    @staticmethod
    def unpack(hd):
        """The one copy back of a handle -> {section name: numpy array [B, ...]} (csrc/cocoap.hip's outputs under their names)."""
        hd.event.synchronize()
        host = hd.buf.cpu().numpy()
        out = {}
        for name, (o, dtype, shape) in hd.views.items():
            n = int(np.prod(shape))
            out[name] = host[o:o + n * dtype.itemsize].view(dtype).reshape(shape)
        return out

    def collect(self, hd):
        """One copy back; appends the frame records (a frame without detections and ground truths leaves none) -> the unpacked sections."""
        r = self.unpack(hd)
        for b in range(hd.B):
            n_top, ngp = int(r["counts"][b, 0]), int(r["counts"][b, 1])
            self.frames += 1
            for a in range(len(AREA_RNG)):
                if n_top == 0 and ngp == 0:
                    self.records[a].append(None)
                    continue
                self.records[a].append({"scores": r["scores"][b, :n_top].copy(), "dtm": r["dtm"][b, a, :, :n_top] != 0,
                                        "dtIg": r["dtIg"][b, a, :, :n_top] != 0, "gtIg": r["gi"][b, a][r["gorder"][b, a, :ngp]].copy()})
        self._tables = None
        return r

    def update(self, *args, **kw):
        return self.collect(self.enqueue(*args, **kw))

    # ---- the host half ----
    def accumulate(self):
        """-> (precision [T,R,A,M], recall [T,A,M]) over the collected records."""
        if self._tables is None:
            self._tables = accumulate_records(self.records)
        return self._tables

    def summarize(self):
        """-> stats f64 [12]: AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl; -1 where undefined."""
        return summarize_tables(*self.accumulate())

    def results(self):
        """detectron2's dict (COCOEvaluator._derive_coco_results): the six AP values x 100, NaN where undefined."""
        stats = self.summarize()
        return {k: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, k in enumerate(STAT_NAMES[:6])}
