"""Validation losses on one MI355X: quber_loss_targets and quber_losses (csrc/losses.hip) timed with HIP events around blocks of calls that
rotate over several inputs, their kernels' times and bytes from the library's stage profiler in a run of their own, and the contract
(tests/test_losses_cpu.py: loss_targets_np, losses_ref) on the host of the same box on one frame, compared with the device's result.
A context without a network.  Prints ONE JSON line.

  default        batch 16 at 640x480, 20 ground-truth ids per frame: the targets, and the losses with top_k 1.0 / 0.2 and the boundary
                 head's dice / cross-entropy
  --report THIS.json [BENCH.json ...]   the markdown record (profiles/losses_ab.md); the further files hold the JSON result lines of
                 plain `python bench.py` runs of this commit and of its parent, alternated in one session (the file name tells which:
                 it contains "parent" or it does not)

    python3 tools/losses_ab.py [--blocks 7] [--calls 50] [--warmup 2] [--inputs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, N_GT, PLANES = 16, 480, 640, 20, 8
CASES = (("top_k 1.0, dice", 1.0, "dice"), ("top_k 1.0, cross_entropy", 1.0, "cross_entropy"), ("top_k 0.2, dice", 0.2, "dice"),
         ("top_k 0.2, cross_entropy", 0.2, "cross_entropy"))


def timed(call, a):
    import torch
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
    return [float(np.median(ms)), float(np.min(ms)), float(np.max(ms))]


def staged(eng, call, a):
    eng.profile_begin()
    for i in range(a.calls):
        call(i)
    return {k: {"ms": v["ms"] / a.calls, "bytes": v["bytes"] / a.calls, "launches": v["launches"] / a.calls} for k, v in eng.profile_end().items()}


def run(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from quber_amd import engine
    from quber_amd.losses import Losses
    from test_losses_cpu import blob_labels, loss_targets_np, losses_ref, spec, target_planes
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "calls": a.calls, "warmup": a.warmup, "inputs": a.inputs, "batch": B,
           "height": H, "width": W, "n_gt": N_GT, "planes": PLANES, "cases": []}
    rng = np.random.default_rng(2024)
    eng = engine.Engine(engine.make_config(H, W, max_batch=B, max_instances=64, with_network=False), "cuda:0")
    ws0 = int(eng.workspace_bytes())
    labels = [torch.from_numpy(np.stack([blob_labels(rng, H, W, N_GT) for _ in range(B)])).cuda() for _ in range(a.inputs)]
    logits = [torch.from_numpy((rng.standard_normal((B, PLANES, H, W)) * 3).astype(np.float32)).cuda() for _ in range(a.inputs)]
    cls = [torch.from_numpy(rng.integers(0, 4, (B, 2, 1, H, W)).astype(np.uint8)).cuda() for _ in range(a.inputs)]
    explicit = [(c == torch.arange(4, dtype=torch.uint8, device="cuda")[None, None, :, None, None]).to(torch.uint8).contiguous() for c in cls]
    opts = Losses()
    tg = [eng.loss_targets(labels[r], N_GT, opts) for r in range(a.inputs)]
    res["workspace_bytes"] = int(eng.workspace_bytes()) - ws0
    out_t = eng.loss_targets(labels[0], N_GT, opts)
    call_t = lambda i: eng.loss_targets(labels[i % a.inputs], N_GT, opts, out_t)
    t_ms = timed(call_t, a)
    t_stages = staged(eng, call_t, a)
    # the contract on the host, frame 0 of input 0
    lab0 = labels[0][0].cpu().numpy()
    t0 = time.time()
    want = loss_targets_np(lab0, N_GT, opts.sigma, opts.small_area, opts.small_weight, legacy_f32=bool(eng.qcfg.encode_legacy_f32))
    host_t = time.time() - t0
    got = eng.loss_targets(labels[0], N_GT, opts)["targets"][0].cpu().numpy()
    res["targets"] = {"ms_per_call": t_ms, "stages": t_stages, "host_frame_s": host_t,
                      "host_equal": bool(np.array_equal(got.view(np.uint32), target_planes(want).view(np.uint32)))}
    for name, top_k, kind in CASES:
        o = Losses(top_k=top_k, eee_boundary_loss_type=kind)
        heads = {"eee_boundary": 4}
        rec = eng.losses(logits[0], tg[0]["targets"], explicit[0], o, heads=heads)
        call = lambda i: eng.losses(logits[i % a.inputs], tg[i % a.inputs]["targets"], explicit[i % a.inputs], o, rec, heads=heads)
        ms = timed(call, a)
        stages = staged(eng, call, a)
        host = eng.losses(logits[0], tg[0]["targets"], explicit[0], o, heads=heads).cpu().numpy()[0]
        t0 = time.time()
        ref = losses_ref(logits[0][0].cpu().numpy(), tg[0]["targets"][0].cpu().numpy(), explicit[0][0].cpu().numpy(),
                         spec(top_k=top_k, heads={"eee_boundary": (4, kind)}))
        host_s = time.time() - t0
        dev_l = o.unpack(host, heads)[0]
        rel = max(abs(dev_l[k] - v) / max(abs(v), 1e-300) for k, v in ref["losses"].items())
        res["cases"].append({"name": name, "ms_per_call": ms, "stages": stages, "host_frame_s": host_s, "max_rel_err": float(rel)})
    eng.close()
    return res


def report(paths):
    lines = lambda p: [json.loads(l) for l in open(p).read().strip().splitlines() if l.startswith("{")]
    T = lines(paths[0])[-1]
    f = lambda m: f"{m[0]:.3f} ({m[1]:.3f} .. {m[2]:.3f})"
    hw, b = T["height"] * T["width"], T["batch"]
    out = ["# Validation losses on the device: `quber_loss_targets` and `quber_losses` per call and per kernel, and the contract on the host", "",
           f"One MI355X (torch device name: {T['device']}); a context without a network; `tools/losses_ab.py`, one session on one box.  Batch {b} at "
           f"{T['width']}x{T['height']}, {T['n_gt']} seeded ground-truth blobs per frame, {T['planes']} logit planes (fg, centre, two offsets, one "
           f"four-class error head), N(0, 3) logits, uniformly random explicit classes.  Device milliseconds per call: HIP events around blocks of "
           f"{T['calls']} calls that rotate over {T['inputs']} different inputs, median (min .. max) of {T['blocks']} blocks after {T['warmup']} blocks of "
           f"warm-up.  The host column, on ONE frame of the same input on the same box: the contract of tests/test_losses_cpu.py (numpy / float64 torch).", "",
           "| call | device, ms per call | device, ms per frame | host contract, s per frame | device against the contract |", "|---|---|---|---|---|",
           f"| targets (sigma 10) | {f(T['targets']['ms_per_call'])} | {T['targets']['ms_per_call'][0] / b:.4f} | {T['targets']['host_frame_s']:.3f} | "
           f"{'bit-equal' if T['targets']['host_equal'] else 'DIFFERENT'} |"]
    for c in T["cases"]:
        out.append(f"| losses, {c['name']} | {f(c['ms_per_call'])} | {c['ms_per_call'][0] / b:.4f} | {c['host_frame_s']:.3f} | max relative error {c['max_rel_err']:.1e} |")
    moved = 4.0 * b * hw * (1 + 6) + b * hw * (4.0 * (T["planes"] + 6) + 4)
    both = T["targets"]["ms_per_call"][0] + T["cases"][0]["ms_per_call"][0]
    out += ["", f"The two calls together (targets + losses at top_k 1.0, dice) move {moved / 1e6:.0f} MB once - the label map in and six target planes out, "
            f"then {T['planes']} logit planes, six target planes and four explicit bytes per pixel in - in {both:.3f} ms: {moved / both / 1e9:.2f} TB/s "
            "achieved (`tta_merge`, a pure streaming kernel, reaches 5.0-5.2 TB/s on record).", "",
            "Per kernel, from the library's stage profiler in a run of its own (an event pair per stage, so the sum exceeds the call above); "
            "bytes are what the stage must read and write once, computed from the shapes by the launcher:", "",
            "| call | stage | ms per call | MB per call | GB/s |", "|---|---|---|---|---|"]
    for name, st in [("targets", T["targets"]["stages"])] + [("losses, " + c["name"], c["stages"]) for c in T["cases"]]:
        for k, s in st.items():
            if not s["launches"]:                        # a stage of an earlier window of this context: nothing of it ran in this one
                continue
            out.append(f"| {name} | {k} | {s['ms']:.4f} | {s['bytes'] / 1e6:.1f} | {s['bytes'] / max(s['ms'], 1e-9) / 1e6:.0f} |")
    out += ["", f"The workspace the first call adds to the context (moments, centres, block partials, histograms, the float64 foreground plane, for "
            f"max_batch frames): {T['workspace_bytes'] / 2 ** 20:.1f} MiB."]
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
