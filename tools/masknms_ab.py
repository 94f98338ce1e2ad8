"""Mask NMS on one MI355X: quber_mask_nms (csrc/masknms.hip) timed with HIP events around blocks of calls that rotate over several
inputs, its kernels' times and bytes from the library's stage profiler in a run of their own, and the numpy contract
(tests/test_masknms_cpu.py: mask_nms_np) on the host of the same box on one frame of each input, compared with the device's result.
A context without a network.  Prints ONE JSON line.

  default        the four cases: batch 16 at 640x480 with 20, 100 and 200 proposals per frame; batch 1 at 1280x720 with 30
  --report THIS.json [BENCH.json ...]   the markdown record (profiles/masknms_ab.md); the further files hold the JSON result lines of
                 plain `python bench.py` runs of this commit and of its parent, alternated in one session (the file name tells which:
                 it contains "parent" or it does not)

    python3 tools/masknms_ab.py [--blocks 7] [--calls 100] [--warmup 2] [--inputs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((16, 480, 640, 20), (16, 480, 640, 100), (16, 480, 640, 200), (1, 720, 1280, 30))
FRAMES = 4                 # distinct seeded frames per case; the batches of the rotating inputs are drawn from them, shifted


def run(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from quber_amd import engine
    from test_masknms_cpu import mask_nms_np, proposals, reference_nms_combine
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "calls": a.calls, "warmup": a.warmup, "inputs": a.inputs, "cases": []}
    for B, H, W, N in CASES:
        sets = [proposals(H, W, N, 1000 + f, distinct=False) for f in range(min(FRAMES, max(B, 2)))]
        frames = torch.from_numpy(np.stack([s[0] for s in sets])).cuda()
        fscores = torch.from_numpy(np.stack([s[1] for s in sets])).cuda()
        # input r: frame b of the batch is seeded frame (b + r) % FRAMES, rolled by 37 (b // FRAMES + 3 r) columns: same statistics,
        # different bytes - no call finds the previous call's planes in a cache under the same addresses
        inputs = []
        for r in range(a.inputs):
            pick = [(b + r) % len(sets) for b in range(B)]
            m = torch.stack([torch.roll(frames[p], 37 * (b // len(sets) + 3 * r), dims=-1) for b, p in enumerate(pick)]).contiguous()
            inputs.append((m, fscores[pick].contiguous()))
        eng = engine.Engine(engine.make_config(H, W, max_batch=B, max_instances=max(N, 1), with_network=False), "cuda:0")
        ws0 = int(eng.lib.quber_workspace_bytes(eng.h))
        outs = {k: v for k, v in eng.mask_nms(*inputs[0]).items()}          # allocates the workspace; the outputs are reused below
        ws1 = int(eng.lib.quber_workspace_bytes(eng.h))
        call = lambda i: eng.mask_nms(inputs[i % a.inputs][0], inputs[i % a.inputs][1], None, outs["masks"], outs["ids"], outs["source"],
                                      outs["scores"], outs["report"])
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
        got = eng.mask_nms(*inputs[0])
        hm, hs = inputs[0][0][0].cpu().numpy(), inputs[0][1][0].cpu().numpy()
        t0 = time.time()
        want = mask_nms_np(hm, hs)
        host_s = time.time() - t0
        t0 = time.time()
        ref = reference_nms_combine(hm, hs)                                  # the reference's own loops: one np.multiply + np.sum per pair
        ref_s = time.time() - t0
        rep = got["report"].cpu().numpy()
        equal = (np.array_equal(got["masks"][0].cpu().numpy(), want[0]) and np.array_equal(got["source"][0].cpu().numpy(), want[2])
                 and np.array_equal(got["ids"][0].cpu().numpy(), want[4]) and rep[0].tolist() == [want[1], want[3], 0, 0])
        res["cases"].append({"batch": B, "height": H, "width": W, "masks": N, "ms_per_call": [float(np.median(ms)), float(np.min(ms)), float(np.max(ms))],
                             "stages": stages, "count_mean": float(rep[:, 0].mean()), "kept_mean": float(rep[:, 1].mean()),
                             "host_frame_s": host_s, "host_equal": bool(equal), "reference_frame_s": ref_s, "reference_masks": len(ref[0]),
                             "workspace_bytes": ws1 - ws0})
        eng.close()
        del frames, inputs, outs, got
    return res


def report(paths):
    lines = lambda p: [json.loads(l) for l in open(p).read().strip().splitlines() if l.startswith("{")]
    T = lines(paths[0])[-1]
    f = lambda m: f"{m[0]:.3f} ({m[1]:.3f} .. {m[2]:.3f})"
    out = ["# Mask NMS on the device: `quber_mask_nms` per call and per kernel, and the numpy contract on the host", "",
           f"One MI355X (torch device name: {T['device']}); a context without a network; `tools/masknms_ab.py`, one session on one box.  Every frame "
           f"holds seeded proposals of a few objects (overlapping blobs, exact and near duplicates, nested parts; scores with ties).  Device "
           f"milliseconds per call: HIP events around blocks of {T['calls']} calls that rotate over {T['inputs']} different inputs, median (min .. max) "
           f"of {T['blocks']} blocks after {T['warmup']} blocks of warm-up.  The host columns, on ONE frame of the same input on the same box: `mask_nms_np`, the contract "
           f"(its pair table is one float32 matrix product), and `reference_nms_combine`, the reference's own loops (one full-frame `np.multiply` + "
           f"`np.sum` per pair), both in tests/test_masknms_cpu.py.", "",
           "| batch | frame | proposals per frame | kept / visible per frame (mean) | device, ms per call | device, ms per frame | host contract, s per frame | "
           "reference's loops, s per frame | contract equal to the device's result |",
           "|---|---|---|---|---|---|---|---|---|"]
    for c in T["cases"]:
        out.append(f"| {c['batch']} | {c['width']}x{c['height']} | {c['masks']} | {c['kept_mean']:.1f} / {c['count_mean']:.1f} | {f(c['ms_per_call'])} | "
                   f"{c['ms_per_call'][0] / c['batch']:.3f} | {c['host_frame_s']:.3f} | {c['reference_frame_s']:.2f} | {'yes' if c['host_equal'] else 'NO'} |")
    out += ["", "Per kernel, from the library's stage profiler in a run of its own (an event pair per stage, so the sum exceeds the call above); "
            "bytes are what the stage must read and write once, computed from the shapes by the launcher (gram: every plane once per tile of "
            "partners, plus the pair table):", "",
            "| case | stage | ms per call | MB per call | GB/s |", "|---|---|---|---|---|"]
    for c in T["cases"]:
        for k, s in c["stages"].items():
            out.append(f"| {c['batch']} x {c['masks']} @ {c['width']}x{c['height']} | {k} | {s['ms']:.4f} | {s['bytes'] / 1e6:.1f} | "
                       f"{s['bytes'] / max(s['ms'], 1e-9) / 1e6:.0f} |")
    out += ["", "The workspace the first call adds to the context (bit planes, pair table, rank map, per-frame tables, for max_batch x max_instances masks): " +
            ", ".join(f"{c['workspace_bytes'] / 2 ** 20:.1f} MiB for {c['batch']} x {c['masks']} @ {c['width']}x{c['height']}" for c in T["cases"]) + "."]
    if len(paths) > 1:
        out += ["", "Plain `python bench.py --gpus 1 --steps 20 --warmup 5 --cpu-frames 0` (the feature is off there: no new kernel runs), this commit and its parent "
                "alternated in one session on one box:", "", "| run | commit | value | unit |", "|---|---|---|---|"]
        vals = {"this": [], "parent": []}
        for p in paths[1:]:
            who = "parent" if "parent" in os.path.basename(p) else "this"
            for j in lines(p):
                if "value" in j:
                    vals[who].append(float(j["value"]))
                    out.append(f"| {os.path.basename(p)} | {who} | {j['value']:.1f} | {j.get('unit', '')} |")
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
    ap.add_argument("--calls", type=int, default=100, help="calls per timed block (one event pair per block)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inputs", type=int, default=3)
    ap.add_argument("--report", nargs="+", metavar="JSON")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    print(json.dumps(run(a)))


if __name__ == "__main__":
    main()
