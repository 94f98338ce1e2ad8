"""Perturbed initial masks on one MI355X: quber_perturb_masks with its bit planes in LDS against the same kernel body with them in
device memory, and against the numpy contract (tests/test_perturb_cpu.py: perturb_np) on the host.  Batch 16 x 20 masks, 640x480,
every mask a seeded ellipse, a context without a network, the programs of Perturb(target, seed=0).  Prints ONE JSON line.

  default        per target (0.95, 0.8, 0.6) the device time of the call between two events in placement 1 (LDS) and 2 (device memory),
                 alternated; the rounds the masks ran; the two placements compared bit for bit; the contract timed on the host for the
                 first --host-masks masks of the batch on the same programs, and compared with the device's result
  --report THIS.json [BENCH.json ...]   the markdown record (profiles/perturb_ab.md); the further files hold the JSON result lines of
                 plain `python bench.py` runs of this commit and of its parent, alternated in one session (the file name tells which)

    python3 tools/perturb_ab.py [--steps 20] [--warmup 3] [--host-masks 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

H, W, N, B = 480, 640, 20, 16
TARGETS = (0.95, 0.8, 0.6)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ellipse_masks():
    """u8 [B,N,H,W]: one seeded axis-aligned ellipse per mask, semi-axes 30..120 x 40..160 px, 255 inside."""
    rng = np.random.RandomState(77)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((B, N, H, W), np.uint8)
    for b in range(B):
        for i in range(N):
            cy, cx, ry, rx = rng.uniform(100, H - 100), rng.uniform(120, W - 120), rng.uniform(30, 120), rng.uniform(40, 160)
            m[b, i] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0) * 255
    return m


def run(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from quber_amd import engine
    from quber_amd.perturb import Perturb
    from test_perturb_cpu import perturb_np
    masks = ellipse_masks()
    t0 = time.time()
    progs = Perturb(0.8, seed=0).programs(B, N, H, W)        # the programs depend on the seeds only: one draw serves every target
    draw_s = time.time() - t0
    eng = engine.Engine(engine.make_config(H, W, max_batch=B, max_instances=N, with_network=False), "cuda:0")
    d_masks, d_progs = torch.from_numpy(masks).cuda(), torch.from_numpy(progs.copy()).cuda()
    outs = [torch.empty_like(d_masks) for _ in (1, 2)]
    reps = [torch.empty((B, N, 4), dtype=torch.int32, device="cuda") for _ in (1, 2)]
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "program_draw_s": draw_s, "targets": {}}
    for target in TARGETS:
        d_tg = torch.full((B, N), target, dtype=torch.float64, device="cuda")
        ms = {1: [], 2: []}
        for i in range(a.warmup + a.steps):
            for placement in (1, 2):                          # alternated: both see the same neighbours on the box
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.perturb_masks(d_masks, d_progs, d_tg, outs[placement - 1], reps[placement - 1], placement)
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    ms[placement].append(e0.elapsed_time(e1))
        rep = reps[0].cpu().numpy().astype(np.int64)
        r = {"same_bits": bool(torch.equal(outs[0], outs[1]) and torch.equal(reps[0], reps[1])),
             "rounds_mean": float(rep[:, :, 0].mean()), "rounds_min": int(rep[:, :, 0].min()), "rounds_max": int(rep[:, :, 0].max()),
             "ops_total": int(rep[:, :, 0].sum() * 4),
             "iou_mean": float((rep[:, :, 1] / np.maximum(rep[:, :, 2], 1)).mean())}
        for placement, name in ((1, "lds_ms"), (2, "device_memory_ms")):
            r[name] = (float(np.median(ms[placement])), float(np.min(ms[placement])), float(np.max(ms[placement])))
        got = outs[0].cpu().numpy()
        k = min(a.host_masks, N)
        t0 = time.time()
        want = [perturb_np(masks[0, i], progs[0, i], target) for i in range(k)]
        r["host_masks"], r["host_s"] = k, time.time() - t0
        r["host_rounds"] = [int(w[1][0]) for w in want]
        r["host_equal"] = all(np.array_equal(got[0, i], w[0]) and np.array_equal(rep[0, i], w[1]) for i, w in enumerate(want))
        res["targets"][str(target)] = r
    eng.close()
    return res


def report(paths):
    last = lambda p: json.loads([l for l in open(p).read().strip().splitlines() if l.startswith("{")][-1])
    T = last(paths[0])
    f = lambda m: f"{m[0]:.3f} ({m[1]:.3f} .. {m[2]:.3f})"
    out = ["# Perturbed initial masks: the bit planes in LDS against device memory, and against numpy on the host", "",
           f"One MI355X (torch device name: {T['device']}); `quber_perturb_masks` on batch {B} x {N} masks, {W}x{H}, every mask a seeded ellipse, the programs "
           f"of `Perturb(target, seed=0)` (250 rounds of 4 operations), a context without a network; device milliseconds per call between two events, "
           f"median (min .. max) of {T['steps']} calls after {T['warmup']}, the two placements alternated call by call; `tools/perturb_ab.py`, one session on one box.", "",
           "| target | rounds per mask, mean (min .. max) | operations in all | mean IoU reached | LDS, ms | device memory, ms | LDS / device memory | same bits |",
           "|---|---|---|---|---|---|---|---|"]
    for t, r in T["targets"].items():
        out.append(f"| {t} | {r['rounds_mean']:.1f} ({r['rounds_min']} .. {r['rounds_max']}) | {r['ops_total']} | {r['iou_mean']:.3f} | {f(r['lds_ms'])} | "
                   f"{f(r['device_memory_ms'])} | {r['lds_ms'][0] / r['device_memory_ms'][0]:.2f} | {'yes' if r['same_bits'] else 'NO'} |")
    out += ["", f"The numpy contract (`perturb_np`) on the host of the same box for the first masks of frame 0, on the same programs; the device time per mask is the "
            f"LDS call's time over its {B * N} masks (they run side by side, so this is throughput, not latency):", "",
            "| target | masks | their rounds | host, s | host, ms per mask | device, ms per mask | equal to the device's result |", "|---|---|---|---|---|---|---|"]
    for t, r in T["targets"].items():
        out.append(f"| {t} | {r['host_masks']} | {r['host_rounds']} | {r['host_s']:.2f} | {1e3 * r['host_s'] / r['host_masks']:.0f} | "
                   f"{r['lds_ms'][0] / (B * N):.4f} | {'yes' if r['host_equal'] else 'NO'} |")
    out += ["", f"Drawing the {B * N} programs on the host (`Perturb.programs`, {B * N * 8000} calls of a `RandomState`): {T['program_draw_s']:.1f} s, once per "
            "(frames, masks, height, width) - they depend on the seeds only and are kept."]
    if len(paths) > 1:
        out += ["", "Plain `python bench.py --gpus 1` (the feature is off there), this commit and its parent alternated in one session:", "",
                "| file | masks/s | ms per step |", "|---|---|---|"]
        for p in paths[1:]:
            for line in open(p).read().strip().splitlines():
                if line.startswith("{"):
                    j = json.loads(line)
                    out.append(f"| {os.path.basename(p)} | {j.get('value')} | {j.get('ms_per_step')} |")
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-masks", type=int, default=20, help="masks of frame 0 the numpy contract is timed on, per target")
    ap.add_argument("--report", nargs="+", metavar="JSON")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    print(json.dumps(run(a)))


if __name__ == "__main__":
    main()
