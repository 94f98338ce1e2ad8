"""The Gaussian mean shift of centre votes on one MI355X: quber_gms_cluster (csrc/gms.hip) timed with HIP events around blocks of calls at
640x480, batch 1 and batch 16, with the reference's settings (200 seeds, 10 rounds, subsample 5, IMP 9); the IMP pass alone; and the two
baselines a user has today on the same inputs: the numpy contract on the host (tests/test_gms_cpu.py: gms_np) and the reference's loops
restated as torch on the device (multinomial seeding, the S x n_sub weight matrix materialised, host loops for the linking and the
IMP left out).  A context without a network.  Prints ONE JSON line; --out writes the markdown record (profiles/gms_ab.md).

    python3 tools/gms_ab.py [--blocks 5] [--calls 10] [--out profiles/gms_ab.md] [--bench THIS.json PARENT.json] [--ratios TESTLOG]

--bench: files with the JSON result lines of plain `python bench.py` runs of this commit and of its parent, alternated in one session.
--ratios: the output of `pytest tests/test_gpu_gms.py -s`, whose "climb ..." lines carry the error ratios."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, K, N_MASKS = 480, 640, 6, 32


def scene(seed):
    """All of a 640x480 frame but a background band votes for one of K centres; 1 % salt, so that the IMP has work."""
    rng = np.random.RandomState(seed)
    centres = np.array([[0.25 * j - 0.6, 0.1 * (j % 2) - 0.05, 0.8 + 0.05 * j] for j in range(K)])
    yy, xx = np.mgrid[:H, :W]
    which = np.clip(((xx + 12 * np.sin(yy / 17.0 + seed)) * K / W).astype(int), 0, K - 1)
    salt = rng.rand(H, W) < 0.01
    which[salt] = rng.randint(0, K, int(salt.sum()))
    votes = (centres[which].transpose(2, 0, 1) + 0.003 * rng.randn(3, H, W)).astype(np.float32)
    fg = np.ones((H, W), np.uint8)
    fg[:40] = 0
    return np.ascontiguousarray(votes), fg


def torch_reference(votes, fg, g):
    """The reference's method as plain torch on device tensors, one frame (cluster.py / segmentation.py:129-187 restated)."""
    import torch
    X = votes.permute(1, 2, 0)[fg.bool()]
    Xs = X[::g.subsample]
    picked = [torch.randint(0, len(Xs), (1,), device=X.device)[0]]
    nearest = torch.norm(Xs - Xs[picked[0]], dim=1)
    for _ in range(1, g.num_seeds):
        j = torch.multinomial(nearest, 1)[0]
        picked.append(j)
        nearest = torch.minimum(nearest, torch.norm(Xs - Xs[j], dim=1))
    Z = Xs[torch.stack(picked)]
    for _ in range(g.iters):
        Wm = torch.exp(-.5 / g.sigma ** 2 * torch.norm(Z.unsqueeze(1) - Xs.unsqueeze(0), dim=2) ** 2)
        Z = torch.mm(Wm / Wm.sum(dim=1, keepdim=True), Xs)
    from test_gms_cpu import link_np
    sl = torch.from_numpy(link_np(Z.cpu().numpy(), g.epsilon).astype(np.int64)).to(X.device)
    lab = sl[torch.argmin(torch.norm(X.unsqueeze(1) - Z.unsqueeze(0), dim=2), dim=1)]
    return torch.bincount(lab)


def timed(call, a):
    import torch
    for i in range(a.calls):
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
    from quber_amd.gms import GaussianMeanShift
    from test_gms_cpu import gms_np
    g = GaussianMeanShift()
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "calls": a.calls, "cases": []}
    frames = [scene(s) for s in range(3)]
    first, draws = GaussianMeanShift(seed=1).draws([g.n_sub(int(f.sum())) for _, f in frames])
    t0 = time.perf_counter()
    want = gms_np(frames[0][0], frames[0][1], first[0], draws[0], g, N_MASKS)
    res["numpy_contract_s"] = time.perf_counter() - t0
    res["count"], res["imp_changed_pixels"] = int(want["report"][0]), int((want["ids"] != want["raw_ids"]).sum())
    dv, df = [torch.from_numpy(v).cuda() for v, _ in frames], [torch.from_numpy(f).cuda() for _, f in frames]
    res["torch_device_ms"] = timed(lambda i: torch_reference(dv[i % 3], df[i % 3], g), argparse.Namespace(calls=2, blocks=3))
    for B in (1, 16):
        eng = engine.Engine(engine.make_config(H, W, max_batch=B, max_instances=64, with_network=False), "cuda:0")
        sel = [[(i + b) % 3 for b in range(B)] for i in range(3)]
        ins = [(torch.stack([dv[j] for j in s]), torch.stack([df[j] for j in s]), torch.from_numpy(first[s]).cuda(),
                torch.from_numpy(draws[s].view(np.int32)).cuda()) for s in sel]
        out = eng.gms(*ins[0], g, N_MASKS)
        same = bool(np.array_equal(out["ids"][0].cpu().numpy(), want["ids"]))
        case = {"batch": B, "ids_equal_contract": same, "chain_ms": timed(lambda i: eng.gms(*ins[i % 3], g, N_MASKS, out=out), a)}
        no_imp = GaussianMeanShift(imp=None)
        case["chain_without_imp_ms"] = timed(lambda i: eng.gms(*ins[i % 3], no_imp, N_MASKS, out=out), a)
        raw = out["raw_ids"].clone()
        work = raw.clone()

        def imp(i):
            work.copy_(raw)
            eng.gms_imp(work, N_MASKS, g.imp, N_MASKS, masks=out["masks"])
        case["imp_alone_ms"] = timed(imp, a)
        case["copy_ms"] = timed(lambda i: work.copy_(raw), a)
        res["cases"].append(case)
        eng.close()
    return res


def report(res, a):
    lines = ["# Gaussian mean shift of centre votes on one MI355X (tools/gms_ab.py)", "",
             "640x480, %d objects, every pixel below a 40-row background band foreground (n = %d, n_sub = %d), 200 seeds, 10 rounds, "
             "sigma 0.02, subsample 5, min_pixels 300, IMP 9 x 9 + largest component; %d planes.  HIP events around blocks of %d calls that "
             "rotate over 3 inputs, median (min .. max) of %d blocks, per CALL." % (K, (H - 40) * W, -(-(H - 40) * W // 5), N_MASKS, res["calls"],
                                                                                 res["blocks"]), "",
             "Device: %s.  The contract's frame 0 has %d masks; the IMP changes %d pixels of it." % (res["device"], res["count"],
                                                                                                   res["imp_changed_pixels"]), "",
             "| batch | chain (ms) | chain without IMP (ms) | IMP alone incl. a copy of the map (ms) | that copy (ms) | ids == contract |",
             "|---|---|---|---|---|---|"]
    f = lambda t: "%.3f (%.3f .. %.3f)" % tuple(t)
    for c in res["cases"]:
        lines.append("| %d | %s | %s | %s | %s | %s |" % (c["batch"], f(c["chain_ms"]), f(c["chain_without_imp_ms"]), f(c["imp_alone_ms"]),
                                                         f(c["copy_ms"]), c["ids_equal_contract"]))
    lines += ["", "Baselines on the same inputs, one frame: the numpy contract on the host %.2f s; the reference's loops as torch on the device "
              "(multinomial seeding, weight matrix materialised, linking on the host, no IMP) %s ms." % (res["numpy_contract_s"],
                                                                                                        f(res["torch_device_ms"])), ""]
    if a.ratios and os.path.exists(a.ratios):
        rows = re.findall(r"climb (\d+x\d+) frame (\d): err (\S+), e_ref (\S+), ulp (\S+), ratio (\S+)", open(a.ratios).read())
        lines += ["Climb error against the float64 statement (tests/test_gpu_gms.py; the bar is ratio <= 4, ratio = err / max(e_ref, ulp)):", "",
                  "| shape | frame | err | e_ref (torch float32, CPU) | ulp | ratio |", "|---|---|---|---|---|---|"]
        lines += ["| %s | %s | %s | %s | %s | %s |" % r for r in rows] + [""]
    if a.bench:
        vals = []
        for path in a.bench:
            vals.append([json.loads(l)["value"] for l in open(path) if l.startswith("{")])
        lines += ["bench.py headline (refined masks/s, `python bench.py --gpus 1 --steps 20 --warmup 5 --cpu-frames 0`), this commit and its parent alternated on one box: "
                  "this %s, parent %s.  The feature is off by default; the README's box-to-box spread is 10 000 - 10 230." %
                  (", ".join("%.0f" % v for v in vals[0]), ", ".join("%.0f" % v for v in vals[1])), ""]
    else:
        lines += ["bench.py against the parent: not measured in this run.", ""]
    lines += ["Not measured: the split of the chain into seeds / climb / link / assign (the stage profiler's tags gms_* exist; no run of its "
              "own was made), a predictor call with `cluster=` against one fed masks, frames other than 640x480, graph replay.", ""]
    open(a.out, "w").write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--bench", nargs=2)
    ap.add_argument("--ratios")
    ap.add_argument("--from-json", help="write the record from a saved JSON line instead of measuring")
    a = ap.parse_args()
    res = json.loads(open(a.from_json).read()) if a.from_json else run(a)
    if a.out:
        report(res, a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
