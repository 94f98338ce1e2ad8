#!/usr/bin/env python3
"""Batched evaluation beside the per-frame loop it replaces, in one process: multilabel_metrics_batch (csrc/evalbatch.hip, one enqueue
and one copy back for B pairs) against B calls of multilabel_metrics (two synchronisations and a host Munkres per frame), at 640x480
with 18 objects per map from synth.make_masks, B = 16 and B = 32, in alternating blocks.  Device times by HIP events: the whole
batched call with and without the boundary stage (their difference is the boundary stage), and the solver alone on the same score
matrices.  Prints a markdown report (profiles/evalbatch_ab.md is one such run)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quber_amd import _lib, synth                                                # noqa: E402
from quber_amd.eval import evaluation as ev                                      # noqa: E402


def pairs(B, h, w, n, seed):
    preds, gts = np.zeros((B, h, w), np.int32), np.zeros((B, h, w), np.int32)
    for b in range(B):
        gtm, initm = synth.make_masks(np.random.default_rng(seed + b), n, h, w)
        for i in range(n):
            gts[b][gtm[i]] = i + 1
            preds[b][initm[i]] = i + 1
    return preds, gts


def device_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def med(xs):
    q = statistics.quantiles(xs, n=4) if len(xs) >= 4 else [min(xs), statistics.median(xs), max(xs)]
    return f"{statistics.median(xs):.3f} ({q[0]:.3f}-{q[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--objects", type=int, default=18)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    h, w, cap = 480, 640, 64
    lib = _lib.load()
    lines = ["# Batched evaluation against the per-frame loop", "",
             f"640x480, {args.objects} objects per map (`synth.make_masks`), cap {cap}, boundary measures on, {args.reps} alternating blocks;"
             " ms as median (quartiles).", "",
             "| B | batched call, enqueue -> dicts | per frame | per-frame loop of B calls | per frame | ratio |", "|---|---|---|---|---|---|"]
    stage_lines = ["", "Device time of one batched call by events (ms):", "",
                   "| B | whole call | without boundary (labels + score + solver + gather) | boundary stage (difference) | solver alone |", "|---|---|---|---|---|"]
    for B in (16, 32):
        preds, gts = pairs(B, h, w, args.objects, 100)
        exp = [ev.multilabel_metrics(p, g, 0, 1) for p, g in zip(preds[:2], gts[:2])]                 # warm-up + sanity: same dicts
        got = ev.multilabel_metrics_batch(preds, gts, cap=cap)
        assert got.fallback == {} and all(float(got[i][k]) == float(exp[i][k]) for i in range(2) for k in exp[i])
        t_batch, t_loop = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.multilabel_metrics_batch(preds, gts, cap=cap)
            t_batch.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for p, g in zip(preds, gts):
                ev.multilabel_metrics(p, g, 0, 1)
            t_loop.append((time.perf_counter() - t0) * 1e3)
        mb, ml = statistics.median(t_batch), statistics.median(t_loop)
        lines.append(f"| {B} | {med(t_batch)} | {mb / B:.3f} | {med(t_loop)} | {ml / B:.3f} | {ml / mb:.1f}x |")
        dp, dg = torch.from_numpy(preds).cuda(), torch.from_numpy(gts).cuda()
        whole = device_ms(lambda: ev.enqueue_metrics(dp, dg, True, cap), args.reps)
        nobnd = device_ms(lambda: ev.enqueue_metrics(dp, dg, False, cap), args.reps)
        _, tables = ev.multilabel_metrics_batch(preds, gts, cap=cap, return_tables=True)
        score = np.zeros((B, cap, cap))
        for b, t in enumerate(tables):
            score[b, :t["F"].shape[0], :t["F"].shape[1]] = t["F"].max() - t["F"]
        d_score = torch.from_numpy(score).cuda()
        rows = torch.tensor([t["F"].shape[0] for t in tables], dtype=torch.int32, device="cuda")
        cols = torch.tensor([t["F"].shape[1] for t in tables], dtype=torch.int32, device="cuda")
        assign = torch.empty((B, cap), dtype=torch.int32, device="cuda")
        status = torch.empty(B, dtype=torch.int32, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        solver = device_ms(lambda: _lib.check(lib.quber_munkres_batch(p(d_score), p(rows), p(cols), B, cap, 0, None, p(assign), p(status),
                                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))), args.reps)
        stage_lines.append(f"| {B} | {med(whole)} | {med(nobnd)} | {statistics.median(whole) - statistics.median(nobnd):.3f} | {med(solver)} |")
    text = "\n".join(lines + stage_lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
