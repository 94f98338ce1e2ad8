"""The predicted-error-map kernels (csrc/errhead.hip) on one MI355X: prints ONE JSON line (and writes it to --out).

  kernels:  per shape (batch 16 at 640x480 with N = 20 masks; batch 1 at 1280x720 with N = 30; 4 classes) and per kernel
            (error_decode, error_mask_hist, error_score, error_overlay): device milliseconds per launch (HIP events around blocks of
            launches, median over the blocks), the algorithmic bytes computed from the shapes, GB/s and the share of the 6.3 TB/s the
            microarchitecture guide gives as achievable HBM bandwidth; beside each, in the same process and alternating block by
            block, the torch expression a user writes today.  Launches rotate over enough buffer sets (>= 512 MB of inputs per
            kernel) that nothing is served from the 256 MiB last-level cache.  The HIP and torch results are compared once.
  step:     the batch-16 enqueue_batch / collect_batch step at 640x480, N = 20, with decode_errors off and on (alternating rounds,
            device milliseconds between the step's own events): what the flag adds to a step.

    python3 tools/error_decode_bench.py [--launches 200] [--block 20] [--steps 10] [--rounds 3] [--out profiles/r22_error_decode.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quber_amd import arch, engine, synth  # noqa: E402
from quber_amd.eval import error_maps as em  # noqa: E402
from quber_amd.maskrefiner.predictor import RefinerModel  # noqa: E402

HBM_ACHIEVABLE = 6.3e12      # bytes / s
CACHE_BYTES = 512e6          # inputs a rotation must cover: twice the last-level cache
CENTER_BIAS = -1.68          # loud heads with ~N instances per frame (tools/tta_bench.py)
DEV = "cuda:0"


def timed_pair(hip, ref, sets, launches, block, warmup=10):
    """hip(i) / ref(i) launch once on buffer set i % sets.  -> (ms per hip launch, ms per ref launch): medians over alternating blocks."""
    for i in range(warmup):
        hip(i % sets)
        ref(i % sets)
    torch.cuda.synchronize()
    out = {"hip": [], "ref": []}
    k = 0
    for _ in range(max(1, launches // block)):
        for name, fn in (("hip", hip), ("ref", ref)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(block):
                fn(k % sets)
                k += 1
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / block)
    return float(np.median(out["hip"])), float(np.median(out["ref"])), [float(min(out["hip"])), float(max(out["hip"]))]


def row(ms, ref_ms, spread, nbytes, ref_expr, sets):
    return {"ms": ms, "ms_min_max": spread, "bytes": nbytes, "GB_per_s": nbytes / ms * 1e-6, "share_of_6.3TBps": nbytes / (ms * 1e-3) / HBM_ACHIEVABLE,
            "torch_ms": ref_ms, "torch_over_hip": ref_ms / ms, "torch_expression": ref_expr, "buffer_sets": sets}


def kernels(H, W, B, N, launches, block):
    C, first, planes = 4, 4, 8
    hw = H * W
    eng = engine.Engine(engine.make_config(H, W, max_batch=B, max_instances=N, with_network=False), DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    nsets = lambda per_set: max(2, int(np.ceil(CACHE_BYTES / per_set)))
    res = {}

    # ---- error_decode ----
    sl = nsets(B * C * hw * 4)                   # the planes a launch reads: half of a set
    logits = [torch.randn((B, planes, H, W), generator=g, device=DEV) for _ in range(sl)]
    cls = torch.empty((B, H, W), dtype=torch.uint8, device=DEV)
    hist = torch.empty((B, C), dtype=torch.int32, device=DEV)
    frame = (torch.arange(B, device=DEV) * C)[:, None, None]
    t_out = {}

    def t_decode(i):
        c = logits[i][:, first:first + C].argmax(1)
        t_out["cls"] = c.to(torch.uint8)
        t_out["hist"] = torch.bincount((c + frame).view(-1), minlength=B * C).view(B, C)

    ms, rms, sp = timed_pair(lambda i: eng.error_decode(logits[i], (first, C), cls, hist), t_decode, sl, launches, block)
    eng.error_decode(logits[0], (first, C), cls, hist)
    t_decode(0)
    assert torch.equal(cls, t_out["cls"]) and torch.equal(hist.long(), t_out["hist"])
    res["error_decode"] = row(ms, rms, sp, (4 * C + 1) * B * hw, "logits[:, 4:8].argmax(1).to(torch.uint8); torch.bincount(classes + 4 * frame)", sl)
    del logits

    # ---- error_mask_hist ----
    sm = nsets(B * N * hw)
    masks = []
    for s in range(sm):
        m = np.stack([synth.make_scene(100 * s + b, H, W, N)["masks"] for b in range(B)]) if s < 2 else None
        masks.append(torch.from_numpy(m).to(DEV) if m is not None else masks[s % 2].roll(s, 0).contiguous())
    clss = [torch.randint(0, C, (B, H, W), generator=g, device=DEV, dtype=torch.uint8) for _ in range(sm)]
    mh = torch.empty((B, N, C), dtype=torch.int32, device=DEV)

    def t_mask_hist(i):
        inside = masks[i] != 0
        t_out["mh"] = torch.stack([(inside & (clss[i] == c)[:, None]).sum((2, 3)) for c in range(C)], -1)

    ms, rms, sp = timed_pair(lambda i: eng.error_mask_hist(clss[i], masks[i], C, mh), t_mask_hist, sm, launches, block)
    eng.error_mask_hist(clss[0], masks[0], C, mh)
    t_mask_hist(0)
    assert torch.equal(mh.long(), t_out["mh"])
    res["error_mask_hist"] = row(ms, rms, sp, B * hw * (N + 1) + 4 * B * N * C, "((masks != 0) & (classes == c)[:, None]).sum((2, 3)) for c in range(4)", sm)

    # ---- error_score ----
    se = nsets(B * 5 * hw)
    expl = [eng.error_maps(masks[i % sm], masks[(i + 1) % sm]) for i in range(se)]
    cl2 = [torch.randint(0, C, (B, H, W), generator=g, device=DEV, dtype=torch.uint8) for _ in range(se)]
    table = torch.empty((B, C + 1, C), dtype=torch.int64, device=DEV)
    frame2 = (torch.arange(B, device=DEV) * (C + 1) * C)[:, None, None]

    def t_score(i):
        tgt = expl[i][:, 1].argmax(1)              # e3: the explicit planes are one-hot, no pixel without a target
        t_out["table"] = torch.bincount((tgt * C + cl2[i] + frame2).view(-1), minlength=B * (C + 1) * C).view(B, C + 1, C)

    ms, rms, sp = timed_pair(lambda i: eng.error_score(cl2[i], expl[i], 1, "e3", table), t_score, se, launches, block)
    eng.error_score(cl2[0], expl[0], 1, "e3", table)
    t_score(0)
    assert torch.equal(table, t_out["table"])
    res["error_score"] = row(ms, rms, sp, 5 * B * hw + 8 * B * (C + 1) * C, "torch.bincount(explicit[:, 1].argmax(1) * 4 + classes + 20 * frame)", se)
    del expl, masks

    # ---- error_overlay ----
    so = nsets(B * 7 * hw)
    bgr = [torch.randint(0, 256, (B, H, W, 3), generator=g, device=DEV, dtype=torch.uint8) for _ in range(so)]
    cl3 = [clss[i % sm] for i in range(so)]
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=DEV)
    pal = em.DEFAULT_PALETTE["e3"]
    cols = {c: torch.tensor(p, dtype=torch.uint8, device=DEV) for c, p in enumerate(pal) if p is not None}

    def t_overlay(i):
        o = bgr[i].clone()
        for c, col in cols.items():
            o[cl3[i] == c] = col
        t_out["vis"] = o

    ms, rms, sp = timed_pair(lambda i: eng.error_overlay(bgr[i], cl3[i], pal, out), t_overlay, so, launches, block)
    eng.error_overlay(bgr[0], cl3[0], pal, out)
    t_overlay(0)
    assert torch.equal(out, t_out["vis"])
    res["error_overlay"] = row(ms, rms, sp, 7 * B * hw, "vis = bgr.clone(); vis[classes == c] = colour[c] for c in (TP, FP, FN)", so)
    eng.close()
    return res


def step_cost(steps, rounds, warmup=3):
    H, W, B, N = 480, 640, 16, 20
    sd = arch.init_state_dict(seed=0, loud_heads=True, center_bias=CENTER_BIAS)
    batch = synth.make_batch(9, B, H, W, N)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    bgr, dep, masks = d(batch["rgb"]), d(batch["depth"]), d(batch["masks"])
    model = RefinerModel(None, sd, DEV)
    ms = {False: [], True: []}
    keys = {}
    for r in range(rounds + 1):
        for flag in (False, True):
            model.decode_errors = flag
            for s in range(warmup if r == 0 else steps):
                outs, t = model.collect_batch(model.enqueue_batch(bgr, dep, masks, slots=N + 12))
                if r > 0:
                    ms[flag].append(t)
            keys[flag] = sorted(k for k in outs[0] if k != "instances")
    model.close()
    off, on = float(np.median(ms[False])), float(np.median(ms[True]))
    q = lambda v: [float(np.percentile(v, 25)), float(np.percentile(v, 75))]
    return {"shape": f"batch {B}, {W}x{H}, N={N}", "ms_off": off, "ms_on": on, "ms_off_quartiles": q(ms[False]), "ms_on_quartiles": q(ms[True]),
            "added_ms": on - off, "added_share_of_step": (on - off) / off, "steps_per_flag": len(ms[False]), "keys_off": keys[False],
            "keys_on": keys[True]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("error_decode_bench needs a ROCm GPU: nothing here is measured on a CPU")
    out = {
        "metric": "predicted error maps on the device: decode, per-mask attribution, confusion table, overlay (4 classes)",
        "timing": f"HIP events around blocks of {a.block} launches, {a.launches} launches per kernel, HIP and torch blocks alternating; median block",
        "kernels": {"b16_640x480_n20": kernels(480, 640, 16, 20, a.launches, a.block),
                    "b1_1280x720_n30": kernels(720, 1280, 1, 30, a.launches, a.block)},
        "step": step_cost(a.steps, a.rounds),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
