"""Boundary AP on one MI355X: one CocoAP.enqueue + collect under "segm" and under "boundary" (csrc/boundaryap.hip + csrc/cocoap.hip:
quber_coco_match_boundary, one copy back) at 640x480 x batch 16 with 100 detections x 20 ground truths per frame (the seeded blobs of
tools/cocoap_ab.py; dilation distance 16), inputs resident on the device, against the numpy contract on the host of the same box
(tests/test_boundary_ap_cpu.py: mask_boundary_np; tests/test_cocoap_cpu.py: coco_eval_img_np) on the first --host-frames frames.
Prints ONE JSON line.

  default             wall time per enqueue + collect and device time per enqueue (HIP events) of both types, alternated; the host
                      contract per frame; whether device and host agree record by record and IoU by IoU
  --calls-only N      N "boundary" calls and nothing else: the program to put behind `rocprofv3 --kernel-trace --stats -d DIR --`, in a run
                      of its own
  --report THIS.json [kernel_stats.csv]   the markdown tables (profiles/boundary_ap_ab.md)

    python3 tools/boundary_ap_ab.py [--reps 15] [--warmup 3] [--host-frames 16]
"""
import argparse
import csv
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cocoap_ab import B, H, W, N_DT, N_GT, scene  # noqa: E402


def host_frame(dt, scores, gt, flags, d, contract, bcontract):
    """The contract on one frame: the boundaries by mask_boundary_np, both sets as bit planes (np.packbits), inter by np.bitwise_and +
    np.bitwise_count, the float64 IoU expressions, their minimum, coco_eval_img_np per area range -> (records, mask iou, boundary iou)."""
    order = np.argsort(-scores, kind="mergesort")[:100]
    crowd = (flags & 1) != 0

    def table(a, b):
        pa, pb = np.packbits(a.reshape(len(a), -1) != 0, axis=1), np.packbits(b.reshape(len(b), -1) != 0, axis=1)
        aa, ab = np.bitwise_count(pa).sum(1, dtype=np.int64), np.bitwise_count(pb).sum(1, dtype=np.int64)
        iou = np.zeros((len(a), len(b)), np.float64)
        for k in order:
            inter = np.bitwise_count(pa[k][None] & pb).sum(1, dtype=np.int64)
            union = np.where(crowd, aa[k], aa[k] + ab - inter)
            iou[k] = np.where(inter == 0, 0.0, inter.astype(np.float64) / np.maximum(union, 1).astype(np.float64))
        return iou, aa, ab

    iou_m, da, ga = table(dt, gt)
    iou_b = table(np.stack([bcontract.mask_boundary_np(m, d) for m in dt]), np.stack([bcontract.mask_boundary_np(m, d) for m in gt]))[0]
    iou = np.minimum(iou_m, iou_b)
    recs = [contract.coco_eval_img_np(scores, da.astype(np.float64), ga.astype(np.float64), crowd, (flags & 2) != 0, iou, rng) for rng in contract.AREA_RNG]
    return recs, iou_m[order], iou_b[order]


def run(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import test_boundary_ap_cpu as bcontract
    import test_cocoap_cpu as contract
    from quber_amd.eval.coco_ap import CocoAP, boundary_dilation
    frames = [scene(100 + b) for b in range(B)]
    dev = lambda k: torch.from_numpy(np.stack([f[k] for f in frames])).cuda()
    dt, scores, gt, flags = dev(0), dev(1), dev(2), dev(3)
    d = boundary_dilation(H, W)
    aps = {"segm": CocoAP("segm"), "boundary": CocoAP("boundary")}
    if a.calls_only:
        for _ in range(a.calls_only):
            aps["boundary"].collect(aps["boundary"].enqueue(dt, scores, gt, gt_flags=flags))
        return {"calls": a.calls_only}
    wall, devms, last = {k: [] for k in aps}, {k: [] for k in aps}, {}
    for i in range(a.warmup + a.reps):
        for kind, ap in aps.items():                     # alternated: both types see the same state of the box
            ap.reset()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            hd = ap.enqueue(dt, scores, gt, gt_flags=flags)
            e1.record()
            last[kind] = ap.collect(hd)                  # (ends in the copy back: the device work is complete)
            t1 = time.perf_counter()
            if i >= a.warmup:
                wall[kind].append((t1 - t0) * 1e3)
                devms[kind].append(e0.elapsed_time(e1))
    nh = min(a.host_frames, B)
    t0 = time.perf_counter()
    host = [host_frame(*f, d, contract, bcontract) for f in frames[:nh]]
    host_ms = (time.perf_counter() - t0) * 1e3
    ap, r = aps["boundary"], last["boundary"]
    equal = all(np.array_equal(h[0][x][k], ap.records[x][b][k]) for b, h in enumerate(host) for x in range(4) for k in ("scores", "dtm", "dtIg", "gtIg"))
    equal_iou = all(np.array_equal(h[1], r["mask_iou"][b]) and np.array_equal(h[2], r["boundary_iou"][b]) for b, h in enumerate(host))
    same_mask_iou = r["mask_iou"].tobytes() == last["segm"]["iou"].tobytes()
    q = lambda v: [float(np.median(v)), float(np.percentile(v, 25)), float(np.percentile(v, 75))]
    return {"device": torch.cuda.get_device_name(0), "box": platform.node(), "batch": B, "height": H, "width": W, "n_dt": N_DT, "n_gt": N_GT,
            "dilation": d, "reps": a.reps, "warmup": a.warmup, "wall_ms": {k: q(v) for k, v in wall.items()},
            "device_ms": {k: q(v) for k, v in devms.items()}, "host_contract_ms": host_ms, "host_frames": nh, "equal": bool(equal),
            "equal_iou": bool(equal_iou), "mask_iou_equals_segm": bool(same_mask_iou),
            "stats": {k: [float(x) for x in v.summarize()] for k, v in aps.items()}, "record_bytes": int(hd.buf.numel())}


def report(paths):
    T = [json.loads(l) for l in open(paths[0]).read().strip().splitlines() if l.startswith("{")][-1]
    f = lambda m: f"{m[0]:.3f} ({m[1]:.3f}-{m[2]:.3f})"
    yes = lambda v: "yes" if v else "NO"
    out = [f"{T['width']}x{T['height']} x batch {T['batch']}, {T['n_dt']} detections x {T['n_gt']} ground truths per frame (seeded blobs, two crowds), "
           f"dilation distance {T['dilation']}; `tools/boundary_ap_ab.py` on one MI355X (torch device name: {T['device']}; box {T['box']}).  Inputs "
           f"resident on the device; {T['reps']} calls of each type after {T['warmup']} of warm-up, the two types alternated, ms as median (quartiles).", "",
           "| what | `segm`, ms per batch | `boundary`, ms per batch |", "|---|---|---|",
           f"| `enqueue + collect`, wall time of the calling thread (launches, the one copy back, records unpacked) | {f(T['wall_ms']['segm'])} | {f(T['wall_ms']['boundary'])} |",
           f"| the launches of `enqueue` alone, HIP events | {f(T['device_ms']['segm'])} | {f(T['device_ms']['boundary'])} |", "",
           f"The numpy contract on the host of the same box (`mask_boundary_np` on every mask, `np.packbits`, `np.bitwise_and` + `np.bitwise_count`, "
           f"`coco_eval_img_np`) on the first {T['host_frames']} frames: {T['host_contract_ms']:.0f} ms, {T['host_contract_ms'] / T['host_frames']:.0f} ms per frame.  "
           f"On those frames the records of the two paths are equal (scores, dtm, dtIg, gtIg of every area range): {yes(T['equal'])}; the mask IoU and "
           f"boundary IoU tables are equal bit for bit: {yes(T['equal_iou'])}; `mask_iou` of the boundary call equals `iou` of the segm call over the "
           f"whole batch: {yes(T['mask_iou_equals_segm'])}.", "",
           f"The twelve numbers of this input, segm: {', '.join('%.4f' % x for x in T['stats']['segm'])}; "
           f"boundary: {', '.join('%.4f' % x for x in T['stats']['boundary'])}."]
    if len(paths) > 1:
        rows = [r for r in csv.DictReader(open(paths[1])) if any(k in r["Name"] for k in ("ca_", "zero_kernel"))]
        out += ["", "Per launch of the `boundary` type, `rocprofv3 --kernel-trace --stats` in a run of its own (the same input, `--calls-only`):", "",
                "| kernel | calls | average, us | share of all kernel time |", "|---|---|---|---|"]
        for r in rows:
            out.append(f"| `{r['Name'].split('(')[0]}` | {r['Calls']} | {float(r['AverageNs']) / 1e3:.1f} | {float(r['Percentage']):.1f} % |")
    print("\n".join(out))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--host-frames", type=int, default=B)
    p.add_argument("--calls-only", type=int, default=0)
    p.add_argument("--report", nargs="+", metavar="FILE")
    a = p.parse_args()
    if a.report:
        return report(a.report)
    print(json.dumps(run(a)))


if __name__ == "__main__":
    main()
