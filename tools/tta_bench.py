"""Horizontal-flip test-time augmentation on one MI355X at 640x480: prints ONE JSON line.

  predict_b1:   MaskRefinerPredictor.predict() ms per call (median), plain and tta=True, N = 20 initial masks
  batch16:      masks/s of the resident-input step at batch 16, N = 20 (bench.py's step: encode + forward + post-processing + mask
                extraction), plain and with TTA (flip + encode + one forward of 32 frames + merge + post-processing + extraction)
  stages:       the tta_flip / tta_merge stages of the batch-16 TTA step from the stage profiler (ms, algorithmic bytes, GB/s) and
                their share of that step
  equivariance: TTA(flip(x)) against flip(TTA(x)) (x-offset negated) at batch 1: max |d| and whether it is bit-exact

    python3 tools/tta_bench.py [--steps 10] [--warmup 3] [--calls 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quber_amd import arch, engine, synth  # noqa: E402
from quber_amd.maskrefiner.predictor import MaskRefinerPredictor, RefinerModel  # noqa: E402

H, W, N = 480, 640, 20
CENTER_BIAS = -1.68          # loud heads with ~N instances per frame (tests/test_gpu_network.py: test_adapter_stream_batched)


def predict_ms(sd, tta, scene, calls, warmup):
    pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, tta=tta)
    for _ in range(warmup):
        out = pred.predict(scene["rgb"], scene["depth"], scene["masks"])
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pred.predict(scene["rgb"], scene["depth"], scene["masks"])[0]
        if "instances" in out:
            out["instances"].to("cpu")
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    k = len(out["instances"]) if "instances" in out else 0
    pred.model.close()
    return float(np.median(ts)), k


def batch_run(sd, tta, batch, steps, warmup):
    B = 16
    f = 2 if tta else 1
    dev = "cuda:0"
    eng = engine.Engine(engine.make_config(H, W, max_batch=f * B, max_instances=N), dev)
    eng.load_state_dict(sd)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    bgr = torch.empty((f * B, H, W, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty_like(bgr)
    masks = torch.empty((f * B, N, H, W), dtype=torch.uint8, device=dev)
    bgr[:B].copy_(d(batch["rgb"]))
    depth[:B].copy_(d(batch["depth"]))
    masks[:B].copy_(d(batch["masks"]))
    offsets = torch.empty((f * B, 3, H, W), dtype=torch.float32, device=dev)
    logits = torch.empty((B, eng.planes, H, W), dtype=torch.float32, device=dev)
    post = eng.alloc_post(B)
    max_inst = min(eng.cap, N + 12)
    om = torch.empty((B, max_inst, H, W), dtype=torch.uint8, device=dev)

    def step():
        if tta:
            eng.tta_flip_inputs(bgr, depth, masks)
            eng.encode(masks, offsets)
            eng.tta_merge(eng.forward(bgr, depth, offsets), logits)
        else:
            eng.encode(masks, offsets)
            eng.forward(bgr, depth, offsets, logits)
        eng.postprocess(logits, post)
        eng.extract_masks(post, max_inst, om)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    runs = []
    for _ in range(3):
        eng.profile_begin()
        step()
        runs.append(eng.profile_end())
    stages = {k: dict(runs[0][k], ms=float(np.median([r[k]["ms"] for r in runs]))) for k in runs[0]}
    total = sum(v["ms"] for v in stages.values())
    out = {"masks_per_s": B * N * steps / el, "ms_per_step": el / steps * 1e3, "stage_ms_sum": total,
           "instances_out_per_frame_mean": float(post["count"].float().mean())}
    if tta:
        for k in ("tta_flip", "tta_merge"):
            s = stages[k]
            out[k] = {"ms": s["ms"], "bytes": s["bytes"], "launches": s["launches"], "GB_per_s": s["bytes"] / s["ms"] * 1e-6,
                      "share_of_step": s["ms"] / total}
    eng.close()
    return out


def equivariance(sd, scene):
    eng = engine.Engine(engine.make_config(H, W, max_batch=2, max_instances=N), "cuda:0")
    eng.load_state_dict(sd)
    model = RefinerModel(None, sd, "cuda:0", tta=True)

    def run(rgb, dep, m):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate([a[None], a[None]])))
        return model.tta_logits(eng, t(rgb).cuda(), t(dep).cuda(), t(m).cuda()).cpu().numpy()

    a = run(scene["rgb"], scene["depth"], scene["masks"])
    f = run(np.flip(scene["rgb"], 1), np.flip(scene["depth"], 1), np.flip(scene["masks"], 2))
    f = np.array(f[..., ::-1])
    f[:, 3] = -f[:, 3]
    eng.close()
    return {"max_abs": float(np.abs(f - a).max()), "bit_exact": bool(np.array_equal(f.view(np.uint32), a.view(np.uint32))),
            "max_abs_logit": float(np.abs(a).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=30)
    a = ap.parse_args()
    sd = arch.init_state_dict(seed=0, loud_heads=True, center_bias=CENTER_BIAS)
    scene = synth.make_scene(5, H, W, N)
    plain_ms, k0 = predict_ms(sd, False, scene, a.calls, a.warmup)
    tta_ms, k1 = predict_ms(sd, True, scene, a.calls, a.warmup)
    batch = synth.make_batch(9, 16, H, W, N)
    b_plain = batch_run(sd, False, batch, a.steps, a.warmup)
    b_tta = batch_run(sd, True, batch, a.steps, a.warmup)
    out = {
        "metric": f"horizontal-flip TTA at {W}x{H} RGB-D, N={N}",
        "predict_b1": {"plain_ms": plain_ms, "tta_ms": tta_ms, "ratio": tta_ms / plain_ms, "instances": [k0, k1]},
        "batch16": {"plain": b_plain, "tta": b_tta, "masks_per_s_ratio": b_tta["masks_per_s"] / b_plain["masks_per_s"]},
        "equivariance_b1": equivariance(sd, scene),
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
