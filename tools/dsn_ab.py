"""A/B of the Depth Seeding Network forward at 480 x 640 (profiles/dsn_ab.md): ms per forward at batch 1 and batch 8 of
  (a) the restatement tests/dsn_torch.py run by PyTorch-ROCm eager on the same GPU - how the reference runs the network,
  (b) the HIP plan with option key 53 (dsn_fused) = 0: an ESP module's five dilated convolutions from the convolution launchers + esp_merge,
  (c) the HIP plan with dsn_fused = 1: esp_branches.
The three arms alternate inside every round (a, b, c, a, b, c, ...), each timed over `--iters` forwards between two device
synchronisations after a warm-up; the table gives the median over the rounds and the spread (min .. max).  Then, per HIP arm, one
forward with an event pair around every op (DsnEngine.profile, median of `--rounds` such forwards per op): the share of the three ESP
modules (reduce convolution .. GroupNorm) and the head kernel's time against the 64-channel float32 feature map it reads.

    python tools/dsn_ab.py [--rounds 7] [--iters 10] [--out profiles/dsn_ab.md]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dsn_torch as D                                              # noqa: E402
from quber_amd import dsn_arch                                     # noqa: E402
from quber_amd.seeding import DsnEngine                            # noqa: E402

H, W = 480, 640
ARMS = ("a eager torch", "b dsn_fused=0", "c dsn_fused=1")


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dsn_ab needs the GPU: a CPU timing says nothing about it")
    sd = dsn_arch.init_state_dict(0)
    wdev = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    lines = ["| batch | arm | launches (ops) | median ms / forward | min .. max | ratio to eager |", "|---|---|---|---|---|---|"]
    shares, verdict = [], {}
    for B in a.batches:
        x = torch.from_numpy(np.stack([D.synth_xyz(H, W, 50 + i) for i in range(B)])).cuda()
        engines = {f: DsnEngine(sd, H, W, B, fused=f) for f in (0, 1)}
        nops = {f: len(e.eng.plan()) for f, e in engines.items()}
        nlaunch = {f: sum(p[3] for p in e.eng.plan()) for f, e in engines.items()}

        def eager():
            with torch.no_grad():
                return D.forward(x, wdev)

        arms = dict(zip(ARMS, (eager, lambda: engines[0].forward(x), lambda: engines[1].forward(x))))
        ref = eager()                                   # same results first: the three arms agree to the network's tolerance
        for f in (0, 1):
            got = engines[f].forward(x)
            err = max(float((g - r).abs().max()) for g, r in zip(got, ref))
            assert err < 1e-4, (B, f, err)
        for fn in arms.values():                        # warm-up of every arm at this shape
            timed(fn, 3)
        ms = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                ms[k].append(timed(fn, a.iters))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k in arms:
            info = "-" if k.startswith("a") else "%d (%d)" % (nlaunch[int(k[-1])], nops[int(k[-1])])
            lines.append("| %d | %s | %s | %.3f | %.3f .. %.3f | %.2f |" % (B, k, info, med[k], min(ms[k]), max(ms[k]), med[ARMS[0]] / med[k]))
        verdict[B] = (ms, med)
        for f in (0, 1):                                # per op: the ESP modules' share and the head
            runs = [engines[f].profile(x) for _ in range(a.rounds)]
            names = [n for n, _ in runs[0]]
            per_op = np.median(np.array([[t for _, t in r] for r in runs]), 0)
            total = float(per_op.sum())
            esp = {m: float(sum(t for n, t in zip(names, per_op) if n.startswith(m + "."))) for m in D.ESP}
            head = float(per_op[names.index("head")])
            shares.append("| %d | dsn_fused=%d | %.3f | %s | %.1f %% | %.3f | %.0f GB/s |" % (
                B, f, total, " / ".join("%.3f" % esp[m] for m in D.ESP), 100.0 * sum(esp.values()) / total, head,
                B * H * W * 64 * 4 / (head * 1e-3) / 1e9))
        for e in engines.values():
            e.close()
    lines.append("")
    for B, (ms, med) in verdict.items():
        c_beats_a = max(ms[ARMS[2]]) < min(ms[ARMS[0]])
        c_beats_b = max(ms[ARMS[2]]) < min(ms[ARMS[1]])
        b_beats_c = max(ms[ARMS[1]]) < min(ms[ARMS[2]])
        lines.append("batch %d: fused faster than eager beyond the spread: %s (x%.2f); fused faster than unfused beyond the spread: %s; unfused faster than "
                     "fused beyond the spread: %s (unfused / fused x%.2f)" % (B, c_beats_a, med[ARMS[0]] / med[ARMS[2]], c_beats_b, b_beats_c, med[ARMS[1]] / med[ARMS[2]]))
    lines += ["", "Per op (event pairs around every op, one stream, median of the rounds): the three ESP modules from their reduce convolution to their",
              "GroupNorm, and the head kernel against the %.1f MB of features per frame it reads:" % (H * W * 64 * 4 / 1e6), "",
              "| batch | plan | sum of the ops, ms | layer3b / layer4b / fuse_layer, ms | ESP share | head, ms | head read rate |", "|---|---|---|---|---|---|---|"] + shares
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
