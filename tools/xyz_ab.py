"""A/B of the two ways into the Depth Seeding Network at 480 x 640 (profiles/xyz_ab.md), batch 1 and batch 8:
  (x) forward(xyz = a host array f32 [B,3,H,W]): the caller back-projected on the host (not timed); upload of 12 bytes per pixel, dsn_pack first,
  (z) forward(z = a host array f32 [B,H,W], camera=): upload of 4 bytes per pixel, the fused back-projection + pack first
      (csrc/dsn.hip xyz_from_depth_kernel), in both conventions.
Both include the upload from pageable host memory (torch.from_numpy(...).to(device)) and the whole forward.  The arms alternate inside
every round (x, z pinhole, z uois, x, ...), each timed over `--iters` calls between two device synchronisations after a warm-up; the table
gives the median over the rounds and the spread (min .. max).  Then the first op alone, from DsnEngine.profile's event pair around it
(it also clears the GroupNorm sums in every arm), and the upload alone.

    python tools/xyz_ab.py [--rounds 7] [--iters 10] [--out profiles/xyz_ab.md]
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
from quber_amd.camera import Camera, xyz_np                        # noqa: E402
from quber_amd.seeding import DsnEngine                            # noqa: E402

H, W = 480, 640
ARMS = ("x xyz= (host xyz)", "z camera= pinhole", "z camera= uois")


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
    ap.add_argument("--feature-dim", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xyz_ab needs the GPU: a CPU timing says nothing about it")
    sd = dsn_arch.init_state_dict(0, feature_dim=a.feature_dim)
    cams = {ARMS[1]: Camera(570.3, 570.3, 319.5, 239.5), ARMS[2]: Camera(570.3, 570.3, 319.5, 239.5, "uois")}
    lines = ["| batch | arm | upload, MB | median ms / call | min .. max | ratio to xyz= |", "|---|---|---|---|---|---|"]
    first, verdict = [], []
    for B in a.batches:
        z = np.ascontiguousarray(np.stack([D.synth_xyz(H, W, 50 + i)[2] for i in range(B)]))            # f32 [B,H,W], NaN pixels
        xyz = np.ascontiguousarray(xyz_np(z, cams[ARMS[1]]).transpose(0, 3, 1, 2))                        # what the caller of xyz= built
        net = DsnEngine(sd, H, W, B)
        up = lambda h: torch.from_numpy(h).to(net.device)
        arms = {ARMS[0]: lambda: net.forward(up(xyz)), ARMS[1]: lambda: net.forward(z=up(z), camera=cams[ARMS[1]]),
                ARMS[2]: lambda: net.forward(z=up(z), camera=cams[ARMS[2]])}
        ref, got = arms[ARMS[0]](), arms[ARMS[1]]()                     # the same bits first
        assert all(torch.equal(r.view(torch.int32), g.view(torch.int32)) for r, g in zip(ref, got)), B
        for fn in arms.values():
            timed(fn, 3)
        ms = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                ms[k].append(timed(fn, a.iters))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k in arms:
            mb = (xyz if k == ARMS[0] else z).nbytes / 1e6
            lines.append("| %d | %s | %.1f | %.3f | %.3f .. %.3f | %.3f |" % (B, k, mb, med[k], min(ms[k]), max(ms[k]), med[ARMS[0]] / med[k]))
        for k in ARMS[1:]:
            verdict.append("batch %d, %s: faster than xyz= beyond the spread: %s; slower beyond the spread: %s (xyz= / camera= x%.3f, %.3f ms per call)" % (
                B, k, max(ms[k]) < min(ms[ARMS[0]]), min(ms[k]) > max(ms[ARMS[0]]), med[ARMS[0]] / med[k], med[ARMS[0]] - med[k]))
        # the first op alone (event pair), and the upload alone (host clock around copy + synchronise)
        dx, dz = up(xyz), up(z)
        ops = {ARMS[0]: lambda: net.profile(dx), ARMS[1]: lambda: net.profile(z=dz, camera=cams[ARMS[1]]), ARMS[2]: lambda: net.profile(z=dz, camera=cams[ARMS[2]])}
        per = {k: [] for k in ops}
        for _ in range(a.rounds):
            for k, fn in ops.items():
                r = fn()
                assert r[0][0] == "pack"
                per[k].append(r[0][1])
        ups = {"xyz": [], "z": []}
        for _ in range(a.rounds):
            for k, h in (("xyz", xyz), ("z", z)):
                ups[k].append(timed(lambda: up(h), a.iters))
        for k in ops:
            u = ups["xyz" if k == ARMS[0] else "z"]
            first.append("| %d | %s | %.4f | %.4f .. %.4f | %.3f | %.3f .. %.3f |" % (B, k, float(np.median(per[k])), min(per[k]), max(per[k]),
                                                                                 float(np.median(u)), min(u), max(u)))
        net.close()
    lines += [""] + verdict
    lines += ["", "The first op of the plan alone (clears the GroupNorm sums, then dsn_pack or the fused back-projection + pack; one event pair, median of",
              "the rounds) and the upload alone (host clock around the copy from pageable memory and a synchronisation):", "",
              "| batch | arm | first op, ms | min .. max | upload, ms | min .. max |", "|---|---|---|---|---|---|"] + first
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
