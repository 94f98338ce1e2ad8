"""Iterative refinement on one MI355X: batch 16, 640x480 RGB-D, N = 20 initial masks, exact fp32, loud weights.  Prints ONE JSON line.

  --chain-host   uses only calls that exist without the feature (enqueue_batch / collect_batch of an iterations=1 model), so it also
                 runs on a checkout of an earlier commit (--root DIR: import quber_amd from there):
                   one_pass_device_ms     (a) one pass, device milliseconds between the events of enqueue_batch
                   chain3_wall_ms         (b) three passes chained through the host: refined masks to the host, uint8 * 255, back
                                          to the device, wall time per batch
  default        this commit:
                   loop3_device_ms / loop3_wall_ms   three passes with iterations=3 (wall: the final masks copied to the host, as in (b))
                   stages                 the stage profile of one iterations=3 + track_initial step: the three kernels of
                                          csrc/iterate.hip (ms per launch, algorithmic bytes, GB/s) and the encoding stages
                   mask_overlap           overlap_masks next to error_mask_hist on the same masks, stand-alone
  --report A.json B.json   the markdown record (profiles/iterate_ab.md) from a --chain-host line (A) and a default line (B)

    python3 tools/iterate_bench.py [--chain-host] [--root DIR] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

H, W, N, B = 480, 640, 20, 16
CENTER_BIAS = -1.68          # loud heads with ~N instances per frame (tools/tta_bench.py)
HBM_TBS = 8.0


def setup(root):
    sys.path.insert(0, os.path.abspath(root) if root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from quber_amd import arch, synth
    from quber_amd.maskrefiner.predictor import RefinerModel
    sd = arch.init_state_dict(seed=0, loud_heads=True, center_bias=CENTER_BIAS)
    batch = synth.make_batch(9, B, H, W, N)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return torch, RefinerModel, sd, (d(batch["rgb"]), d(batch["depth"]), d((batch["masks"] != 0).astype(np.uint8))), d


def timed(torch, fn, steps, warmup):
    """-> (median device ms as fn reports it, median wall ms, last result)"""
    dev_ms, wall = [], []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms, res = fn()
        torch.cuda.synchronize()
        if i >= warmup:
            dev_ms.append(ms)
            wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(dev_ms)), float(np.median(wall)), res


def chain_host(a):
    torch, RefinerModel, sd, (bgr, dep, masks), d = setup(a.root)
    model = RefinerModel(None, sd, "cuda:0")

    def one():
        outs, ms, host = model.collect_batch(model.enqueue_batch(bgr, dep, masks), host_masks=True)
        return ms, (outs, host)

    def chain():
        total, m = 0.0, masks
        for p in range(3):
            outs, ms, host = model.collect_batch(model.enqueue_batch(bgr, dep, m), host_masks=True)
            total += ms
            if p < 2:                                    # what a caller does between two calls
                n = max([len(x) for x in host] + [1])
                mk = np.zeros((B, n, H, W), np.uint8)
                for b, x in enumerate(host):
                    if len(x):
                        mk[b, :len(x)] = np.asarray(x).astype(np.uint8) * 255
                m = d(mk)
        return total, (outs, host)

    a_ms, a_wall, _ = timed(torch, one, a.steps, a.warmup)
    c_ms, c_wall, (outs, host) = timed(torch, chain, a.steps, a.warmup)
    model.close()
    return {"mode": "chain-host", "one_pass_device_ms": a_ms, "one_pass_wall_ms": a_wall, "chain3_device_ms_sum": c_ms,
            "chain3_wall_ms": c_wall, "instances_per_frame_mean": float(np.mean([len(x) for x in host])),
            "device": torch.cuda.get_device_name(0)}


def loop(a):
    torch, RefinerModel, sd, (bgr, dep, masks), d = setup(a.root)

    def run(m):
        outs, ms, host = m.collect_batch(m.enqueue_batch(bgr, dep, masks), host_masks=True)
        return ms, (outs, host)

    model = RefinerModel(None, sd, "cuda:0")
    a_ms, a_wall, _ = timed(torch, lambda: run(model), a.steps, a.warmup)
    model.close()
    model = RefinerModel(None, sd, "cuda:0", iterations=3)
    l_ms, l_wall, (outs, host) = timed(torch, lambda: run(model), a.steps, a.warmup)
    model.close()
    # the stage profile of one step with everything on
    model = RefinerModel(None, sd, "cuda:0", iterations=3, track_initial=True)
    run(model)
    eng = model.engine_for(H, W, B, N)
    profs = []
    for _ in range(3):
        eng.profile_begin()
        run(model)
        profs.append(eng.profile_end())
    stages = {}
    for k in ("iterate_relabel", "iterate_overlap_ids", "iterate_overlap_masks", "encode_reduce", "encode_label_reduce", "encode_paint"):
        s = profs[0][k]
        ms = float(np.median([p[k]["ms"] for p in profs]))
        stages[k] = {"ms": ms, "launches": s["launches"], "ms_per_launch": ms / s["launches"], "bytes": s["bytes"],
                     "GB_per_s": s["bytes"] / ms * 1e-6, "share_of_8TBs": s["bytes"] / ms * 1e-9 / HBM_TBS}
    step_ms = float(np.median([sum(v["ms"] for v in p.values()) for p in profs]))
    # overlap_masks next to error_mask_hist: same masks, same reading pattern
    cls = (torch.arange(B * H * W, device="cuda:0") // 97 % 4).to(torch.uint8).view(B, H, W)
    ids = (torch.arange(B * H * W, device="cuda:0").view(B, H, W) // 41 % (N + 1)).to(torch.int32)
    hd = model.enqueue_batch(bgr, dep, masks)
    real_ids = eng.relabel_panoptic(hd.post)
    model.collect_batch(hd)
    pair = {}
    for name, fn in (("error_mask_hist", lambda: eng.error_mask_hist(cls, masks, 4)),
                     ("iterate_overlap_masks", lambda: eng.overlap_masks(masks, real_ids, eng.cap)),
                     ("iterate_overlap_masks_synthetic_ids", lambda: eng.overlap_masks(masks, ids, eng.cap))):
        fn()
        ms = []
        for _ in range(5):
            eng.profile_begin()
            fn()
            p = eng.profile_end()
            key = name if name in p else "iterate_overlap_masks"
            ms.append(p[key]["ms"])
        pair[name] = {"ms": float(np.median(ms)), "bytes": p[key]["bytes"], "GB_per_s": p[key]["bytes"] / float(np.median(ms)) * 1e-6}
    model.close()
    return {"mode": "loop", "one_pass_device_ms": a_ms, "one_pass_wall_ms": a_wall, "loop3_device_ms": l_ms, "loop3_wall_ms": l_wall,
            "loop3_over_3x_one_pass": l_ms / (3 * a_ms), "refine_converged_at": [o["refine_converged_at"] for o in outs],
            "instances_per_frame_mean": float(np.mean([len(x) for x in host])), "profiled_step_ms_sum": step_ms, "stages": stages,
            "mask_overlap": pair, "device": torch.cuda.get_device_name(0)}


def report(pa, pb):
    A, L = (json.loads(open(p).read().strip().splitlines()[-1]) for p in (pa, pb))
    f = lambda x: f"{x:.2f}"
    out = ["# Iterative refinement: three passes on the device against three passes through the host", "",
           f"{L['device']}; batch {B}, {W}x{H} RGB-D, N = {N} initial masks, exact fp32, loud weights (~{L['instances_per_frame_mean']:.1f} refined "
           "instances per frame); medians; `tools/iterate_bench.py`.", "",
           "| what | commit | ms per batch |", "|---|---|---|",
           f"| (a) one pass, device time | parent | {f(A['one_pass_device_ms'])} |",
           f"| (a) one pass, device time | this | {f(L['one_pass_device_ms'])} |",
           f"| (b) three passes chained through the host, wall time | parent | {f(A['chain3_wall_ms'])} |",
           f"| ... of which device time (sum of the three steps) | parent | {f(A['chain3_device_ms_sum'])} |",
           f"| three passes, `iterations=3`, device time | this | {f(L['loop3_device_ms'])} |",
           f"| three passes, `iterations=3`, wall time | this | {f(L['loop3_wall_ms'])} |", "",
           f"Device time of `iterations=3` = {L['loop3_device_ms'] / (3 * A['one_pass_device_ms']):.3f} x 3 x (a) of the parent "
           f"({L['loop3_over_3x_one_pass']:.3f} x 3 x (a) of this commit); expected <= 1.05.  Wall time {f(L['loop3_wall_ms'])} ms against "
           f"{f(A['chain3_wall_ms'])} ms through the host.", "",
           "Stages of one `iterations=3, track_initial=True` step (stage profiler; algorithmic bytes; 8 TB/s = 1):", "",
           "| stage | launches | ms per launch | MB per launch | GB/s | of 8 TB/s |", "|---|---|---|---|---|---|"]
    for k, s in L["stages"].items():
        out.append(f"| {k} | {s['launches']} | {s['ms_per_launch']:.4f} | {s['bytes'] / s['launches'] * 1e-6:.1f} | {s['GB_per_s']:.0f} | {s['share_of_8TBs']:.3f} |")
    out += ["", "Stand-alone, the same masks (98 MB):", "", "| kernel | ms | GB/s |", "|---|---|---|"]
    for k, s in L["mask_overlap"].items():
        out.append(f"| {k} | {s['ms']:.4f} | {s['GB_per_s']:.0f} |")
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chain-host", action="store_true")
    ap.add_argument("--root", default=None, help="import quber_amd from this checkout instead of the one this file lies in")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--report", nargs=2, metavar=("CHAIN_JSON", "LOOP_JSON"))
    a = ap.parse_args()
    if a.report:
        return report(*a.report)
    print(json.dumps(chain_host(a) if a.chain_host else loop(a)))


if __name__ == "__main__":
    main()
