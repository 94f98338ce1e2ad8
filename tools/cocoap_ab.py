"""COCO AP on one MI355X: one CocoAP.enqueue + collect (csrc/cocoap.hip: quber_coco_match, one copy back) at 640x480 x batch 16 with 100
detections x 20 ground truths per frame, inputs resident on the device, against the numpy contract on the host of the same box
(tests/test_cocoap_cpu.py: coco_eval_img_np) fed by bit-packed planes, np.bitwise_and and a popcount.  Prints ONE JSON line.

  default             wall time per enqueue + collect and device time per enqueue (HIP events), the host contract per batch, and whether
                      the two agree record by record
  --calls-only N      N calls and nothing else: the program to put behind `rocprofv3 --kernel-trace --stats -d DIR --`, in a run of its own
  --report THIS.json [kernel_stats.csv]   the markdown record (profiles/cocoap_ab.md)

    python3 tools/cocoap_ab.py [--reps 15] [--warmup 3]
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
B, H, W, N_DT, N_GT = 16, 480, 640, 100, 20


def scene(seed):
    """20 seeded blobs as ground truths (two of them crowds), 100 detections: shifted, eroded or merged copies of them with scores."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    gt = np.zeros((N_GT, H, W), np.uint8)
    for g in range(N_GT):
        cy, cx, ry, rx = rng.integers(40, H - 40), rng.integers(40, W - 40), rng.integers(12, 90), rng.integers(12, 110)
        gt[g] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    dt = np.zeros((N_DT, H, W), np.uint8)
    for d in range(N_DT):
        m = np.roll(gt[d % N_GT], (rng.integers(-9, 10), rng.integers(-9, 10)), (0, 1))
        if d % 7 == 3:
            m = m | gt[(d + 1) % N_GT]
        dt[d] = m
    flags = np.zeros(N_GT, np.uint8)
    flags[[5, 13]] = 1
    return dt, rng.random(N_DT).astype(np.float32), gt, flags


def host_frame(dt, scores, gt, flags, contract):
    """The contract on one frame: bit planes (np.packbits), inter by np.bitwise_and + np.bitwise_count, the float64 IoU expressions,
    coco_eval_img_np per area range."""
    pd, pg = np.packbits(dt.reshape(len(dt), -1) != 0, axis=1), np.packbits(gt.reshape(len(gt), -1) != 0, axis=1)
    order = np.argsort(-scores, kind="mergesort")[:100]
    da, ga = np.bitwise_count(pd).sum(1, dtype=np.int64), np.bitwise_count(pg).sum(1, dtype=np.int64)
    crowd = (flags & 1) != 0
    iou = np.zeros((len(dt), len(gt)), np.float64)
    for d in order:
        inter = np.bitwise_count(pd[d][None] & pg).sum(1, dtype=np.int64)
        union = np.where(crowd, da[d], da[d] + ga - inter)
        iou[d] = np.where(inter == 0, 0.0, inter.astype(np.float64) / np.maximum(union, 1).astype(np.float64))
    return [contract.coco_eval_img_np(scores, da.astype(np.float64), ga.astype(np.float64), crowd, (flags & 2) != 0, iou, rng) for rng in contract.AREA_RNG]


def run(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import test_cocoap_cpu as contract
    from quber_amd.eval.coco_ap import CocoAP
    frames = [scene(100 + b) for b in range(B)]
    dev = lambda k, dtype=None: torch.from_numpy(np.stack([f[k] for f in frames])).cuda()
    dt, scores, gt, flags = dev(0), dev(1), dev(2), dev(3)
    ap = CocoAP("segm")
    if a.calls_only:
        for _ in range(a.calls_only):
            ap.collect(ap.enqueue(dt, scores, gt, gt_flags=flags))
        return {"calls": a.calls_only}
    wall, devms = [], []
    for i in range(a.warmup + a.reps):
        ap.reset()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        hd = ap.enqueue(dt, scores, gt, gt_flags=flags)
        e1.record()
        ap.collect(hd)                                   # (ends in the copy back: the device work is complete)
        t1 = time.perf_counter()
        if i >= a.warmup:
            wall.append((t1 - t0) * 1e3)
            devms.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    host = [host_frame(*f, contract) for f in frames]
    host_ms = (time.perf_counter() - t0) * 1e3
    equal = all(np.array_equal(h[x][k], ap.records[x][b][k]) for b, h in enumerate(host) for x in range(4) for k in ("scores", "dtm", "dtIg", "gtIg"))
    q = lambda v: [float(np.median(v)), float(np.percentile(v, 25)), float(np.percentile(v, 75))]
    return {"device": torch.cuda.get_device_name(0), "box": platform.node(), "batch": B, "height": H, "width": W, "n_dt": N_DT, "n_gt": N_GT,
            "reps": a.reps, "warmup": a.warmup, "wall_ms": q(wall), "device_ms": q(devms), "host_contract_ms": host_ms, "equal": bool(equal),
            "stats": [float(x) for x in ap.summarize()], "record_bytes": int(hd.buf.numel())}


def report(paths):
    T = [json.loads(l) for l in open(paths[0]).read().strip().splitlines() if l.startswith("{")][-1]
    f = lambda m: f"{m[0]:.3f} ({m[1]:.3f}-{m[2]:.3f})"
    out = ["# COCO AP: one `enqueue + collect` on the device against the numpy contract on the host", "",
           f"{T['width']}x{T['height']} x batch {T['batch']}, {T['n_dt']} detections x {T['n_gt']} ground truths per frame (seeded blobs, two crowds), segm; "
           f"`tools/cocoap_ab.py` on one MI355X (torch device name: {T['device']}; box {T['box']}).  Inputs resident on the device; "
           f"{T['reps']} calls after {T['warmup']} of warm-up, ms as median (quartiles).", "",
           "| what | ms per batch | ms per frame |", "|---|---|---|",
           f"| `enqueue + collect`, wall time of the calling thread (launches, the one copy back of {T['record_bytes'] / 1024:.0f} KiB, records unpacked) | {f(T['wall_ms'])} | {T['wall_ms'][0] / T['batch']:.3f} |",
           f"| the launches of `enqueue` alone, HIP events | {f(T['device_ms'])} | {T['device_ms'][0] / T['batch']:.3f} |",
           f"| the numpy contract on the host of the same box: `np.packbits`, `np.bitwise_and` + `np.bitwise_count`, `coco_eval_img_np` | {T['host_contract_ms']:.0f} | {T['host_contract_ms'] / T['batch']:.1f} |",
           "", f"Records of the two paths equal (scores, dtm, dtIg, gtIg of every frame and area range): {'yes' if T['equal'] else 'NO'}.  "
           f"The twelve numbers of this input: {', '.join('%.4f' % x for x in T['stats'])}."]
    if len(paths) > 1:
        rows = [r for r in csv.DictReader(open(paths[1])) if any(k in r["Name"] for k in ("ca_", "zero_kernel"))]
        out += ["", "Per launch, `rocprofv3 --kernel-trace --stats` in a run of its own (the same input, `--calls-only`):", "",
                "| kernel | calls | average, us | share of all kernel time |", "|---|---|---|---|"]
        for r in rows:
            out.append(f"| `{r['Name'].split('(')[0]}` | {r['Calls']} | {float(r['AverageNs']) / 1e3:.1f} | {float(r['Percentage']):.1f} % |")
    print("\n".join(out))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--calls-only", type=int, default=0)
    p.add_argument("--report", nargs="+", metavar="FILE")
    a = p.parse_args()
    if a.report:
        return report(a.report)
    print(json.dumps(run(a)))


if __name__ == "__main__":
    main()
