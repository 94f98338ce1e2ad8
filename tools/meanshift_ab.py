"""Mean-shift clustering on one MI355X: quber_meanshift_cluster (csrc/meanshift.hip) and each of its stage entries timed with HIP events
around blocks of calls that rotate over several inputs, the kernels' times from the library's stage profiler in a run of their own,
and the reference's method run as torch on the same device (rocBLAS mm, the S x n weight matrix materialised) on the same inputs.  Also
the climb's error against the float64 statement (tests/test_meanshift_cpu.py: climb_np) beside the error of torch's own float32 mm /
exp on the CPU, per shape.  A context without a network.  Prints ONE JSON line.

  default        640x480, batch 1 and batch 16, 100 seeds, 10 rounds, kappa 20; the error ratio at 24x32, 37x53, 48x64 and 640x480
  --report THIS.json [BENCH.json ...]   the markdown record (profiles/meanshift_ab.md); the further files hold the JSON result lines of
                 plain `python bench.py` runs of this commit and of its parent, alternated in one session (the file name tells which:
                 it contains "parent" or it does not)

    python3 tools/meanshift_ab.py [--blocks 5] [--calls 10] [--warmup 1] [--inputs 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((1, 480, 640), (16, 480, 640))
RATIO_SHAPES = ((24, 32), (37, 53), (48, 64), (480, 640))
RATIO_SEEDS = (1, 2, 31, 32, 33, 100, 128)      # at the three small shapes; 100 alone at 640x480
S, KAPPA, ITERS, N_MASKS = 100, 20.0, 10, 32


def torch_reference(X, first, link_np):
    """The method the reference uses, written as plain torch on device tensors for one frame: X f32 [n,64] -> (indices, climbed seeds,
    labels).  Farthest-first seeds (one rocBLAS matrix-vector product and a running minimum per seed), ten rounds of mean shift with the
    S x n weight matrix materialised (two rocBLAS products and an exp per round), the seeds linked on the host by the contract's link_np
    (in the reference that step is a host loop over numpy too), every pixel to its nearest seed."""
    import torch
    picked = [int(first)]
    nearest = 0.5 * (1 - X @ X[picked[0]])
    for _ in range(1, S):
        j = torch.argmax(nearest)
        picked.append(j)
        nearest = torch.minimum(nearest, 0.5 * (1 - X @ X[j]))
    sel = torch.stack([torch.as_tensor(p, device=X.device) for p in picked])
    Z = X[sel]
    for _ in range(ITERS):
        W = torch.exp(KAPPA * (Z @ X.t()))
        Z = torch.nn.functional.normalize(W @ X, dim=1)
    sl = torch.from_numpy(link_np(Z.cpu().numpy(), 0.04).astype(np.int64)).to(X.device)
    lab = sl[torch.argmin(0.5 * (1 - X @ Z.t()), dim=1)]
    return sel, Z, lab


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


def run(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from quber_amd import engine
    from quber_amd.meanshift import MeanShift
    from test_meanshift_cpu import blob_embeddings, climb_np, link_np, same_partition, seeds_np
    ms_opt = MeanShift(num_seeds=S, kappa=KAPPA, iters=ITERS)
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "calls": a.calls, "warmup": a.warmup, "inputs": a.inputs, "cases": [],
           "ratios": []}
    # the climb against float64, beside torch's float32 on the CPU
    for h, w in RATIO_SHAPES:
        emb, _ = blob_embeddings(h, w, 6, 40 + h)
        X = np.ascontiguousarray(emb.reshape(64, -1).T)
        eng = engine.Engine(engine.make_config(h, w, max_batch=1, max_instances=64, with_network=False), "cuda:0")
        d_emb = torch.from_numpy(emb[None]).cuda()
        Xt = torch.from_numpy(X)
        for ns in (RATIO_SEEDS if h * w <= 4096 else (S,)):
            idx = eng.meanshift_seeds(d_emb, torch.tensor([7], dtype=torch.int32, device="cuda"), ns)
            hidx = idx.cpu().numpy()[0]
            seeds_equal = bool(np.array_equal(hidx, seeds_np(X, 7, ns))) if h * w <= 4096 else None
            got = eng.meanshift_climb(d_emb, indices=idx, kappa=KAPPA, iters=ITERS).cpu().numpy()[0]
            want = climb_np(X, X[hidx], KAPPA, ITERS)
            Z = Xt[torch.from_numpy(hidx.astype(np.int64))]
            for _ in range(ITERS):
                Z = torch.nn.functional.normalize(torch.exp(KAPPA * (Z @ Xt.t())) @ Xt, dim=1)
            e_ref = float(np.abs(Z.numpy().astype(np.float64) - want).max())
            err = float(np.abs(got.astype(np.float64) - want).max())
            res["ratios"].append({"height": h, "width": w, "seeds": ns, "device_error": err, "e_ref": e_ref, "ratio": err / e_ref,
                                  "seeds_equal_contract": seeds_equal})
        eng.close()
    for B, H, W in CASES:
        made = [blob_embeddings(H, W, 5 + f, 900 + f) for f in range(3)]
        frames = torch.from_numpy(np.stack([m[0] for m in made])).cuda()
        inputs = []
        for r in range(a.inputs):           # frame b of input r: seeded frame (b + r) % 3, rolled: same statistics, different bytes
            e = torch.stack([torch.roll(frames[(b + r) % 3], 37 * (b // 3 + 3 * r), dims=-1) for b in range(B)]).contiguous()
            inputs.append((e, torch.randint(0, H * W, (B,), dtype=torch.int32, device="cuda")))
        eng = engine.Engine(engine.make_config(H, W, max_batch=B, max_instances=64, with_network=False), "cuda:0")
        ws0 = int(eng.lib.quber_workspace_bytes(eng.h))
        out = eng.meanshift(inputs[0][0], inputs[0][1], ms_opt, N_MASKS)
        ws1 = int(eng.lib.quber_workspace_bytes(eng.h))
        pick = lambda i: inputs[i % a.inputs]
        t = {"chain": timed(lambda i: eng.meanshift(pick(i)[0], pick(i)[1], ms_opt, N_MASKS, out=out), a),
             "seeds": timed(lambda i: eng.meanshift_seeds(pick(i)[0], pick(i)[1], S, out=out["indices"]), a),
             "climb": timed(lambda i: eng.meanshift_climb(pick(i)[0], out["seeds"], out["indices"], KAPPA, ITERS), a),
             "link": timed(lambda i: eng.meanshift_link(out["seeds"], 0.04, out=out["seed_labels"]), a),
             "assign": timed(lambda i: eng.meanshift_assign(pick(i)[0], out["seeds"], out["seed_labels"], N_MASKS, ids=out["ids"], masks=out["masks"],
                                                            report=out["report"]), a)}
        eng.profile_begin()
        for i in range(a.calls):
            eng.meanshift(pick(i)[0], pick(i)[1], ms_opt, N_MASKS, out=out)
        stages = {k: {"ms": v["ms"] / a.calls, "flops": v.get("flops", 0.0) / a.calls, "launches": v["launches"] / a.calls}
                  for k, v in eng.profile_end().items()}
        # the reference's method as torch on the device, frame by frame as the reference runs it
        rows = lambda e: e.reshape(64, -1).t().contiguous()
        ref = lambda i: [torch_reference(rows(pick(i)[0][b]), pick(i)[1][b], link_np) for b in range(B)]
        small = argparse.Namespace(warmup=1, calls=max(1, a.calls // 5), blocks=3)
        t["torch_reference"] = timed(ref, small)
        r = eng.meanshift(inputs[0][0], inputs[0][1], ms_opt, N_MASKS)
        sel, Z, lab = torch_reference(rows(inputs[0][0][0]), inputs[0][1][0], link_np)
        rep = r["report"].cpu().numpy()
        big = int(torch.bincount(lab).argmax())
        res["cases"].append({"batch": B, "height": H, "width": W, "ms": t, "stages": stages, "workspace_bytes": ws1 - ws0,
                             "count_mean": float(rep[:, 0].mean()),
                             "same_seeds_as_torch": int((sel.cpu().numpy() == r["indices"][0].cpu().numpy()).sum()),
                             "same_partition_as_torch": bool(same_partition(r["ids"][0].cpu().numpy() != 0, (lab != big).cpu().numpy())
                                                             and len(torch.unique(lab)) == rep[0, 1] + 1)})
        eng.close()
        del frames, inputs, out, r
    return res


def report(paths):
    lines = lambda p: [json.loads(l) for l in open(p).read().strip().splitlines() if l.startswith("{")]
    T = lines(paths[0])[-1]
    f = lambda m: f"{m[0]:.3f} ({m[1]:.3f} .. {m[2]:.3f})"
    out = ["# Mean-shift clustering on the device: `quber_meanshift_cluster`, its stages, and the reference's method as torch on the same device", "",
           f"One MI355X (torch device name: {T['device']}); a context without a network; `tools/meanshift_ab.py`, one session on one box.  Every frame "
           f"holds seeded unit embeddings around 5 to 7 directions (float16-representable), {S} seeds, {ITERS} rounds, kappa {KAPPA:g}, {N_MASKS} output planes.  "
           f"Device milliseconds per call: HIP events around blocks of {T['calls']} calls that rotate over {T['inputs']} different inputs, median (min .. max) of "
           f"{T['blocks']} blocks after {T['warmup']} block(s) of warm-up.  `torch, reference's method`: farthest-first seeds, the mean shift and the "
           "assignment written as plain torch on the same device (rocBLAS products, the 100 x n weight matrix materialised ten times), frame by frame, "
           "the linking on the host (a numpy loop in the reference too); fewer calls per block.", "",
           "| batch | frame | chain, ms per call | seeds | climb | link | assign + write | torch, reference's method, ms per call | torch / chain | "
           "masks per frame (mean) | same seeds as torch (of 100, frame 0) | same partition as torch (frame 0) |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in T["cases"]:
        m = c["ms"]
        out.append(f"| {c['batch']} | {c['width']}x{c['height']} | {f(m['chain'])} | {f(m['seeds'])} | {f(m['climb'])} | {f(m['link'])} | {f(m['assign'])} | "
                   f"{f(m['torch_reference'])} | {m['torch_reference'][0] / m['chain'][0]:.1f}x | {c['count_mean']:.1f} | {c['same_seeds_as_torch']} | "
                   f"{'yes' if c['same_partition_as_torch'] else 'NO'} |")
    out += ["", "Per stage of the chain, from the library's stage profiler in a run of its own (an event pair per stage); FLOPs are counted from the shapes "
            "by the launcher (climb: 4 S n 64 per round, the padded seed rows not counted):", "",
            "| case | stage | ms per call | launches per call | GFLOP per call | TFLOP/s |", "|---|---|---|---|---|---|"]
    for c in T["cases"]:
        for k, s in c["stages"].items():
            out.append(f"| {c['batch']} @ {c['width']}x{c['height']} | {k} | {s['ms']:.4f} | {s['launches']:.0f} | {s['flops'] / 1e9:.2f} | "
                       f"{s['flops'] / max(s['ms'], 1e-9) / 1e9:.2f} |")
    out += ["", "The climb against the float64 statement (`climb_np`) on the same float32 inputs, beside `e_ref`, the error of torch's own float32 "
            "`mm` / `exp` on the CPU against the same statement, on one blob frame per shape; tests/test_gpu_meanshift.py allows the device 4 x `e_ref` "
            "(on its own frames - two blob frames and a grid frame per shape, the maximum over the three - it prints its figures when run with `-s`):", "",
            "| frame | seeds | device error (max abs) | e_ref | ratio | seeds equal to the contract |", "|---|---|---|---|---|---|"]
    for r in T["ratios"]:
        eq = "not computed" if r["seeds_equal_contract"] is None else "yes" if r["seeds_equal_contract"] else "NO"
        out.append(f"| {r['width']}x{r['height']} | {r['seeds']} | {r['device_error']:.3e} | {r['e_ref']:.3e} | {r['ratio']:.2f} | {eq} |")
    out += ["", "The workspace the first call adds to the context: " +
            ", ".join(f"{c['workspace_bytes'] / 2 ** 20:.1f} MiB for max_batch {c['batch']} @ {c['width']}x{c['height']}" for c in T["cases"]) + "."]
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
            out += ["", f"This commit: {sp(vals['this'])}.  Parent: {sp(vals['parent'])}.  The median of this commit lies {where} the parent's own "
                    f"run-to-run range ({100 * (np.median(vals['this']) / np.median(vals['parent']) - 1):+.2f} % against the parent's median)."]
    out += ["", "Not measured: the reference's own Python (its seed loop and connected_components as they stand, on its hardware); frames other than "
            "640x480; other seed counts, round counts and kappa; the predictor end to end with `cluster=`; power and clocks during the runs."]
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed block (one event pair per block)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inputs", type=int, default=3)
    ap.add_argument("--report", nargs="+", metavar="JSON")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    print(json.dumps(run(a)))


if __name__ == "__main__":
    main()
