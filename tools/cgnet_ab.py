"""A/B of the CGNet forward at 240 x 320 (profiles/cgnet_ab.md): ms per forward at batch 1 and batch 16 of
  (a) the restatement tests/cgnet_torch.py run by PyTorch-ROCm eager on the same GPU - how the reference runs CGNet,
  (b) the HIP plan with option key 52 (cgnet_fused) = 0: every block from separate launchers,
  (c) the HIP plan with cgnet_fused = 1: cg_joint + cg_apply per block.
The three arms alternate inside every round (a, b, c, a, b, c, ...), each timed over `--iters` forwards between two device
synchronisations after a warm-up; the table gives the median over the rounds and the spread (min .. max).

    python tools/cgnet_ab.py [--rounds 7] [--iters 50] [--out profiles/cgnet_ab.md]
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

import cgnet_torch as G                                            # noqa: E402
from quber_amd import cgnet_arch, synth                            # noqa: E402
from quber_amd.foreground.predictor import CgnetEngine             # noqa: E402

H, W = 240, 320


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cgnet_ab needs the GPU: a CPU timing says nothing about it")
    sd = cgnet_arch.init_state_dict(0)
    wdev = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    lines = ["| batch | arm | launches (ops) | median ms / forward | min .. max | ratio to eager |", "|---|---|---|---|---|---|"]
    verdict = {}
    for B in (1, 16):
        sc = [synth.make_scene(40 + i, H, W, 3) for i in range(B)]
        bgr = torch.from_numpy(np.stack([s["rgb"] for s in sc])).cuda()
        dep = torch.from_numpy(np.stack([s["depth"] for s in sc])).cuda()
        x = torch.cat([G.preprocess(s["rgb"], s["depth"]) for s in sc]).cuda()
        engines = {f: CgnetEngine(sd, H, W, B, fused=f) for f in (0, 1)}
        nops = {f: len(e.eng.plan()) for f, e in engines.items()}
        nlaunch = {f: sum(p[3] for p in e.eng.plan()) + 1 for f, e in engines.items()}       # + the preprocess kernel

        def eager():
            with torch.no_grad():
                return G.forward(x, wdev)

        arms = {"a eager torch": eager, "b cgnet_fused=0": lambda: engines[0].logits(bgr, dep), "c cgnet_fused=1": lambda: engines[1].logits(bgr, dep)}
        # same results first: the three arms agree to the network's tolerance
        ref = eager()
        for f in (0, 1):
            err = float((engines[f].logits(bgr, dep) - ref).abs().max())
            assert err < 1e-4, (B, f, err)
        for fn in arms.values():                        # warm-up of every arm at this shape
            timed(fn, 10)
        ms = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                ms[k].append(timed(fn, a.iters))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k in arms:
            info = "-" if k.startswith("a") else "%d (%d)" % (nlaunch[int(k[-1])], nops[int(k[-1])])
            lines.append("| %d | %s | %s | %.3f | %.3f .. %.3f | %.2f |" % (B, k, info, med[k], min(ms[k]), max(ms[k]), med["a eager torch"] / med[k]))
        verdict[B] = (ms, med)
        for e in engines.values():
            e.eng.close()
    lines.append("")
    for B, (ms, med) in verdict.items():
        c_beats_a = max(ms["c cgnet_fused=1"]) < min(ms["a eager torch"])
        c_beats_b = max(ms["c cgnet_fused=1"]) < min(ms["b cgnet_fused=0"])
        lines.append("batch %d: fused faster than eager beyond the spread: %s (x%.2f); fused faster than unfused beyond the spread: %s (x%.2f)"
                     % (B, c_beats_a, med["a eager torch"] / med["c cgnet_fused=1"], c_beats_b, med["b cgnet_fused=0"] / med["c cgnet_fused=1"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
