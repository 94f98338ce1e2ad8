"""A/B of the Region Refinement Network at 224 x 224 crops (profiles/rrn_ab.md): ms per forward at batch 1 and batch 20 of
  (a) the restatement tests/rrn_torch.py run by PyTorch-ROCm eager on the same GPU - how the reference runs the network,
  (b) the HIP plan with option key 54 (rrn_head) = 0: decoder.last_conv from the convolution launchers, then the 1x1 head kernel,
  (c) the HIP plan with rrn_head = 1: the collapsed 3x3 head, rrn_head3.
The three arms alternate inside every round (a, b, c, a, b, c, ...), each timed over `--iters` forwards between two device
synchronisations after a warm-up; the table gives the median over the rounds and the spread (min .. max).  Then, per HIP arm, one
forward with an event pair around every op (RrnEngine.profile, median of `--rounds` such forwards per op): the slowest ops, and the
head's time against the 64-channel float32 feature map it reads.  Last, the whole stage - ROIs, crop, forward in chunks, paste - for 18
masks on one 480 x 640 frame (RegionRefinement.refine), per arm b and c.

    python tools/rrn_ab.py [--rounds 7] [--iters 5] [--out profiles/rrn_ab.md]
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

import rrn_torch as R                                              # noqa: E402
from quber_amd import engine as qengine, rrn_arch                  # noqa: E402
from quber_amd.region import RegionRefinement, RrnEngine           # noqa: E402

S, FD = 224, 64
ARMS = ("a eager torch", "b rrn_head=0", "c rrn_head=1")


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def stage_scene(h, w, n):
    """n boxes on a grid, a tilted z plane, random bytes -> (bytes u8 [1,h,w,3], ids i32 [1,h,w], z f32 [1,h,w])"""
    rng = np.random.default_rng(1)
    ids = np.zeros((1, h, w), np.int32)
    cols = 6
    for i in range(n):
        y0, x0 = 40 + (i // cols) * 140, 20 + (i % cols) * 100
        ids[0, y0:y0 + int(rng.integers(50, 110)), x0:x0 + int(rng.integers(40, 85))] = i + 1
    ys, xs = np.mgrid[0:h, 0:w]
    z = (0.6 + 0.5 * ys / h + 0.1 * xs / w).astype(np.float32)[None]
    return rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8), ids, z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 20])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rrn_ab needs the GPU: a CPU timing says nothing about it")
    sd = rrn_arch.init_state_dict(0)
    wdev = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    lines = ["| batch | arm | launches (ops) | median ms / forward | min .. max | ratio to eager |", "|---|---|---|---|---|---|"]
    per, verdict = [], {}
    for B in a.batches:
        rgb, mask = (torch.from_numpy(t).cuda() for t in R.synth_crops(B, S, 50))
        engines = {f: RrnEngine(sd, S, B, head=f) for f in (0, 1)}
        nops = {f: len(e.eng.plan()) for f, e in engines.items()}
        nlaunch = {f: sum(p[3] for p in e.eng.plan()) for f, e in engines.items()}

        def eager():
            with torch.no_grad():
                return R.forward(rgb, mask, wdev)

        arms = dict(zip(ARMS, (eager, lambda: engines[0].forward(rgb, mask), lambda: engines[1].forward(rgb, mask))))
        ref = eager()                                   # same results first: the three arms agree to the network's tolerance
        for f in (0, 1):
            err = float((engines[f].forward(rgb, mask) - ref).abs().max())
            assert err < 1e-4, (B, f, err)
        for fn in arms.values():                        # warm-up of every arm at this shape
            timed(fn, 2)
        ms = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                ms[k].append(timed(fn, a.iters))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k in arms:
            info = "-" if k.startswith("a") else "%d (%d)" % (nlaunch[int(k[-1])], nops[int(k[-1])])
            lines.append("| %d | %s | %s | %.3f | %.3f .. %.3f | %.2f |" % (B, k, info, med[k], min(ms[k]), max(ms[k]), med[ARMS[0]] / med[k]))
        verdict[B] = (ms, med)
        for f in (0, 1):                                # per op: the head and the slowest ops
            runs = [engines[f].profile(rgb, mask) for _ in range(a.rounds)]
            names = [n for n, _ in runs[0]]
            per_op = np.median(np.array([[t for _, t in r] for r in runs]), 0)
            total = float(per_op.sum())
            tail = [(n, t) for n, t in zip(names, per_op) if n in ("decoder.last_conv", "head", "head3")]
            head = float(sum(t for _, t in tail))
            kern = float(per_op[names.index("head3" if f else "head")])
            top = sorted(zip(names, per_op), key=lambda p: -p[1])[:4]
            per.append("| %d | rrn_head=%d | %.3f | %s | %.3f | %.3f | %.0f GB/s | %s |" % (
                B, f, total, " + ".join("%s %.3f" % p for p in tail), head, kern, B * S * S * FD * 4 / (kern * 1e-3) / 1e9,
                ", ".join("%s %.3f" % p for p in top)))
        for e in engines.values():
            e.close()
    lines.append("")
    for B, (ms, med) in verdict.items():
        c_beats_b = max(ms[ARMS[2]]) < min(ms[ARMS[1]])
        b_beats_c = max(ms[ARMS[1]]) < min(ms[ARMS[2]])
        lines.append("batch %d: HIP (rrn_head=0) against eager x%.2f; collapsed head faster than convolution + 1x1 beyond the spread: %s; the reverse: %s "
                     "(rrn_head=0 / rrn_head=1 x%.3f)" % (B, med[ARMS[0]] / med[ARMS[1]], c_beats_b, b_beats_c, med[ARMS[1]] / med[ARMS[2]]))
    lines += ["", "Per op (event pairs around every op, one stream, median of the rounds).  tail: what follows decoder.layer5; kernel: the head kernel alone,",
              "and its read rate against the %.1f MB of float32 features per crop it reads (rrn_head3 reads decoder.layer5's output once through LDS tiles" % (S * S * FD * 4 / 1e6),
              "with a halo, rrn_head reads decoder.last_conv's output):", "",
              "| batch | plan | sum of the ops, ms | tail ops, ms | tail, ms | head kernel, ms | its read rate | slowest ops, ms |", "|---|---|---|---|---|---|---|---|"] + per
    # the whole stage on one frame
    h, w, n = 480, 640, 18
    img, ids, z = stage_scene(h, w, n)
    eng = qengine.Engine(qengine.make_config(h, w, max_batch=1, with_network=False))
    d = lambda t: torch.from_numpy(t).cuda()
    d_img, d_ids, d_z = d(img), d(ids), d(z)
    lines += ["", "The whole stage (zoom_rois, rrn_crop, forward in chunks of 20, rrn_paste; the slot list built on the host) for %d masks on one %d x %d frame:" % (n, h, w), "",
              "| plan | median ms / frame | min .. max |", "|---|---|---|"]
    for f in (0, 1):
        region = RegionRefinement(sd, head=f)
        fn = lambda: region.refine(eng, d_img, d_ids, n, [n], d_z)
        timed(fn, 2)
        t = [timed(fn, a.iters) for _ in range(a.rounds)]
        lines.append("| rrn_head=%d | %.3f | %.3f .. %.3f |" % (f, float(np.median(t)), min(t), max(t)))
        region.close()
    eng.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
