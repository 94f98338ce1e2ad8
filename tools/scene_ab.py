"""Scene-level perturbation on one MI355X: quber_scene_perturb (csrc/scene.hip) timed with HIP events around blocks of calls that rotate
over several inputs, its kernels' times and bytes from the library's stage profiler in a run of their own, and the numpy contract
(tests/test_scene_cpu.py: scene_perturb_np) on the host of the same box on one frame of each input, compared with the device's result.
A context without a network.  Prints ONE JSON line.

  default        batch 16 at 640x480, N = 20 ground truths, P = 30 proposals, M = 64: once with the reference's ratio ranges and
                 min_mask_ratio (few decisions act), once with the tests' act probabilities (most do)
  --report THIS.json [BENCH.json ...]   the markdown record (profiles/scene_ab.md); the further files hold the JSON result lines of
                 plain `python bench.py` runs of this commit and of its parent, alternated in one session (the file name tells which:
                 it contains "parent" or it does not)

    python3 tools/scene_ab.py [--blocks 7] [--calls 50] [--warmup 2] [--inputs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, N, P, M = 16, 480, 640, 20, 30, 64
CASES = (("reference ranges, min_mask_ratio 0.01", 0.01, None), ("act 0.6 / 0.6 / 0.4 / 0.6 / 0.2, min_mask_ratio 0.05", 0.05, (0.6, 0.6, 0.4, 0.6, 0.2)))
FRAMES = 4                 # distinct seeded frames; the batches of the rotating inputs are drawn from them, shifted
TABLES = ("fp_act", "gs_act", "merge_act", "split_act", "split_try", "delete_act")


def run(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from quber_amd import engine
    from quber_amd.scene import ScenePerturb
    from test_scene_cpu import random_scene, scene_perturb_np
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "calls": a.calls, "warmup": a.warmup, "inputs": a.inputs,
           "shape": [B, H, W, N, P, M], "cases": []}
    scenes = [random_scene(4000 + f, (H, W), N, P) for f in range(FRAMES)]
    g = torch.from_numpy(np.stack([s["gt"] for s in scenes])).cuda()
    p = torch.from_numpy(np.stack([s["props"] for s in scenes])).cuda()
    n_gt = torch.full((B,), N, dtype=torch.int32, device="cuda")
    n_prop = torch.full((B,), P, dtype=torch.int32, device="cuda")
    for name, ratio, act in CASES:
        opt = ScenePerturb(seed=7, max_masks=M, min_mask_ratio=ratio) if act is None else \
            ScenePerturb(7, M, ratio, *act)
        draws = opt.draws(B, P, H, W)
        d_dev = {k: torch.from_numpy(draws[k].copy()).cuda() for k in TABLES}
        # input r: frame b of the batch is seeded frame (b + r) % FRAMES, rolled by 37 (b // FRAMES + 3 r) columns: same statistics,
        # different bytes - no call finds the previous call's planes in a cache under the same addresses
        inputs = []
        for r in range(a.inputs):
            pick = [(b + r) % FRAMES for b in range(B)]
            roll = lambda t: torch.stack([torch.roll(t[q], 37 * (b // FRAMES + 3 * r), dims=-1) for b, q in enumerate(pick)]).contiguous()
            inputs.append((roll(g), roll(p)))
        eng = engine.Engine(engine.make_config(H, W, max_batch=B, max_instances=M, with_network=False), "cuda:0")
        ws0 = int(eng.lib.quber_workspace_bytes(eng.h))
        outs = eng.scene_perturb(inputs[0][0], inputs[0][1], n_gt, n_prop, d_dev, M, ratio)      # allocates the workspace; the outputs are reused below
        ws1 = int(eng.lib.quber_workspace_bytes(eng.h))
        call = lambda i: eng.scene_perturb(inputs[i % a.inputs][0], inputs[i % a.inputs][1], n_gt, n_prop, d_dev, M, ratio, outs["masks"],
                                           outs["info"], outs["report"])
        for i in range(a.warmup * a.calls):
            call(i)
        torch.cuda.synchronize()
        ms = []
        for blk in range(a.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.calls):
                call(blk * a.calls + i)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.calls)
        # the kernels, in a run of their own (an event pair per stage slows the chain)
        eng.profile_begin()
        for i in range(a.calls):
            call(i)
        stages = {k: {"ms": v["ms"] / a.calls, "bytes": v["bytes"] / a.calls, "launches": v["launches"] / a.calls}
                  for k, v in eng.profile_end().items()}
        # the contract on the host, on frame 0 of input 0, against the device's result for it
        got = call(0)
        torch.cuda.synchronize()
        hg, hp = inputs[0][0][0].cpu().numpy(), inputs[0][1][0].cpu().numpy()
        t0 = time.time()
        want = scene_perturb_np(hg, hp, N, P, M, ratio, {k: v[0] for k, v in draws.items()})
        host_s = time.time() - t0
        rep = got["report"].cpu().numpy()
        equal = (np.array_equal(got["masks"][0].cpu().numpy(), want[0]) and np.array_equal(got["info"][0].cpu().numpy(), want[1])
                 and np.array_equal(rep[0], want[2]))
        res["cases"].append({"name": name, "ms_per_call": [float(np.median(ms)), float(np.min(ms)), float(np.max(ms))], "stages": stages,
                             "report_mean": [float(v) for v in rep.mean(0)], "host_frame_s": host_s, "host_equal": bool(equal),
                             "workspace_bytes": ws1 - ws0, "host_cpus": len(os.sched_getaffinity(0))})
        eng.close()
        del inputs, outs, got
    return res


def report(paths):
    lines = lambda p: [json.loads(l) for l in open(p).read().strip().splitlines() if l.startswith("{")]
    T = lines(paths[0])[-1]
    b, h, w, n, p, m = T["shape"]
    f = lambda v: f"{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})"
    out = ["# Scene-level perturbation on the device: `quber_scene_perturb` per call and per kernel, and the numpy contract on the host", "",
           f"One MI355X (torch device name: {T['device']}); a context without a network; `tools/scene_ab.py`, one session on one box.  Batch {b} at "
           f"{w}x{h}, N = {n} ground truths and P = {p} proposals per frame (seeded ellipses, truncated and grown ground truths: `random_scene` of "
           f"tests/test_scene_cpu.py), M = {m}.  Device milliseconds per call: HIP events around blocks of {T['calls']} calls that rotate over "
           f"{T['inputs']} different inputs, median (min .. max) of {T['blocks']} blocks after {T['warmup']} blocks of warm-up.  The host column, on ONE "
           f"frame of the same input on the same box: `scene_perturb_np`, the contract (boolean numpy; one full-frame pass per pair of masks for the "
           f"overlaps and per pair of list entries for the touch table, as the reference's script has it).  Nobody had measured this stage: no ratio "
           f"was fixed in advance, the two numbers stand beside each other.", "",
           "| draws | list per frame (mean): count, fp, gs, gt kept, absorbed, splits, deleted, dropped | device, ms per call | device, ms per frame | "
           "host contract, s per frame | host CPUs available | contract equal to the device's result |",
           "|---|---|---|---|---|---|---|"]
    for c in T["cases"]:
        out.append(f"| {c['name']} | {', '.join('%.1f' % v for v in c['report_mean'])} | {f(c['ms_per_call'])} | {c['ms_per_call'][0] / b:.4f} | "
                   f"{c['host_frame_s']:.2f} | {c['host_cpus']} | {'yes' if c['host_equal'] else 'NO'} |")
    out += ["", "Per kernel, from the library's stage profiler in a run of its own (an event pair per stage, so the sum exceeds the call above); "
            "bytes are what the stage must read and write once, computed from the shapes by the launcher (upper bounds for the stages that skip "
            "the slots behind the list's length):", "",
            "| draws | stage | ms per call | MB per call |", "|---|---|---|---|"]
    for c in T["cases"]:
        for k, s in c["stages"].items():
            out.append(f"| {c['name']} | {k} | {s['ms']:.4f} | {s['bytes'] / 1e6:.1f} |")
    out += ["", "The workspace the first call adds to the context (source, dilated and composed bit planes, tables, prefix sums): " +
            ", ".join(f"{c['workspace_bytes'] / 2 ** 20:.1f} MiB" for c in T["cases"][:1]) + "."]
    if len(paths) > 1:
        out += ["", "Plain `python bench.py --gpus 1 --steps 20 --warmup 5 --cpu-frames 0` (the feature is off there: no new kernel runs), this commit and its parent "
                "alternated in one session on one box:", "", "| run | commit | value | unit |", "|---|---|---|---|"]
        vals = {"this": [], "parent": []}
        for q in paths[1:]:
            who = "parent" if "parent" in os.path.basename(q) else "this"
            for j in lines(q):
                if "value" in j:
                    vals[who].append(float(j["value"]))
                    out.append(f"| {os.path.basename(q)} | {who} | {j['value']:.1f} | {j.get('unit', '')} |")
        if vals["this"] and vals["parent"]:
            sp = lambda v: f"median {np.median(v):.1f}, {min(v):.1f} .. {max(v):.1f} (spread {100 * (max(v) - min(v)) / np.median(v):.2f} %)"
            med = np.median(vals["this"])
            where = "inside" if min(vals["parent"]) <= med <= max(vals["parent"]) else "ABOVE" if med > max(vals["parent"]) else "BELOW"
            out += ["", f"This commit: {sp(vals['this'])}.  Parent: {sp(vals['parent'])}.  The median of this commit lies "
                    f"{where} the parent's own run-to-run range "
                    f"({100 * (np.median(vals['this']) / np.median(vals['parent']) - 1):+.2f} % against the parent's median)."]
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed block (one event pair per block)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inputs", type=int, default=3)
    ap.add_argument("--report", nargs="+", metavar="JSON")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    print(json.dumps(run(a)))


if __name__ == "__main__":
    main()
