"""Zoom-in refinement on one MI355X: the three entries of csrc/zoom.hip (quber_zoom_rois, quber_zoom_crop, quber_zoom_paste) timed with HIP
events around blocks of calls on a context without a network, the numpy contract (tests/test_zoom_cpu.py) on the host of the same box on
one frame of the same input, compared with the device's result; and a zoomed predict_batch against the plain one, end to end.
Prints ONE JSON line.

  default        batch 16 at 640x480, 18 instances per frame, crop 224; predict_batch of 4 frames at 640x480 with and without zoom
  --report THIS.json [BENCH.json ...]   the markdown record (profiles/zoom_ab.md); the further files hold the JSON result lines of plain
                 `python bench.py` runs of this commit and of its parent, alternated in one session (the file name tells which: it
                 contains "parent" or it does not)

    python3 tools/zoom_ab.py [--blocks 5] [--calls 50] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, N, S, C = 16, 480, 640, 18, 224, 3
FRAMES = 4                 # distinct seeded frames; the batch repeats them


def timed(fn, a, torch):
    for _ in range(a.warmup * a.calls):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / a.calls)
    return [float(np.median(ms)), float(np.min(ms)), float(np.max(ms))]


def run(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    from quber_amd import arch, engine, synth
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
    from quber_amd.zoom import ZoomIn
    from test_zoom_cpu import all_slots, fake_crop_pass, overlap_np, scene, zoom_crop_np, zoom_paste_np, zoom_rois_np
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "blocks": a.blocks, "calls": a.calls, "warmup": a.warmup,
           "case": {"batch": B, "height": H, "width": W, "instances": N, "crop": S}}
    # ---- the three entries ----
    ids4, bgr4, dep4 = scene(H, W, N, 2024, B=FRAMES)
    rep = lambda x: np.concatenate([x] * (B // FRAMES))
    ids, bgr, dep = rep(ids4), rep(bgr4), rep(dep4)
    slots = all_slots(ids, N)
    eng = engine.Engine(engine.make_config(H, W, max_batch=B, max_instances=64, with_network=False), "cuda:0")
    ws0 = int(eng.lib.quber_workspace_bytes(eng.h))
    d_ids, d_bgr, d_dep, d_slots = dev(ids), dev(bgr), dev(dep), dev(slots)
    rois = eng.zoom_rois(d_ids, N, 0.25)
    ws1 = int(eng.lib.quber_workspace_bytes(eng.h))
    crops = eng.zoom_crop(d_bgr, d_dep, d_ids, d_slots, rois, S)
    mc = crops[2].cpu().numpy()
    cid, sc = fake_crop_pass(mc, C, 7)                       # a stand-in for the crop pass: what the paste reads has its shapes and statistics
    table, area = overlap_np(mc, cid, C)
    d_cid, d_sc, d_tab, d_area = dev(cid), dev(sc), dev(table.view(np.int32)), dev(area.view(np.int32))
    final = eng.zoom_paste(d_cid, d_sc, d_tab, d_area, crops[1], d_slots, rois, B, 0.5, 64)
    res["ms"] = {"zoom_rois": timed(lambda: eng.zoom_rois(d_ids, N, 0.25, rois), a, torch),
                 "zoom_crop": timed(lambda: eng.zoom_crop(d_bgr, d_dep, d_ids, d_slots, rois, S, crops), a, torch),
                 "zoom_paste": timed(lambda: eng.zoom_paste(d_cid, d_sc, d_tab, d_area, crops[1], d_slots, rois, B, 0.5, 64, final), a, torch)}
    res["workspace_bytes"] = ws1 - ws0
    rep_dev = final["report"].cpu().numpy()
    res["report_mean"] = [float(v) for v in rep_dev.mean(0)]
    # the contract on the host, on frame 0 alone
    s0 = slots[slots[:, 0] == 0]
    t0 = time.time()
    r_np = zoom_rois_np(ids[:1], N, 0.25)
    t1 = time.time()
    c_np = zoom_crop_np(bgr[:1], dep[:1], ids[:1], s0, r_np, S)
    t2 = time.time()
    p_np = zoom_paste_np(cid[:len(s0)], sc[:len(s0)], table[:len(s0)], area[:len(s0)], c_np[1], s0, r_np, 1, H, W, 0.5, 64)
    t3 = time.time()
    res["host_frame_s"] = {"zoom_rois": t1 - t0, "zoom_crop": t2 - t1, "zoom_paste": t3 - t2}
    res["host_equal"] = bool(np.array_equal(rois[0].cpu().numpy(), r_np[0]) and np.array_equal(crops[0][:len(s0)].cpu().numpy(), c_np[0])
                             and np.array_equal(crops[2][:len(s0)].cpu().numpy(), c_np[2]) and np.array_equal(final["ids"][0].cpu().numpy(), p_np["ids"][0])
                             and np.array_equal(final["masks"][0].cpu().numpy(), p_np["masks"][0]))
    eng.close()
    del d_ids, d_bgr, d_dep, crops, final
    # ---- end to end: predict_batch with and without zoom, loud seeded weights ----
    fb = 4
    scenes = [synth.make_scene(60 + i, H, W, 8) for i in range(fb)]
    rgb, depth = np.stack([s["rgb"] for s in scenes]), np.stack([s["depth"] for s in scenes])
    masks = [s["masks"] for s in scenes]
    sd = arch.init_state_dict(seed=2, loud_heads=True, center_bias=-1.68)
    e2e = {}
    for name, zoom in (("plain", None), ("zoom", ZoomIn(crop=S))):
        pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, zoom=zoom)
        for _ in range(2):
            outs = pred.predict_batch(rgb, depth, masks)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.time()
            outs = pred.predict_batch(rgb, depth, masks)
            torch.cuda.synchronize()
            ts.append((time.time() - t0) * 1e3)
        e2e[name] = {"ms": [float(np.median(ts)), float(min(ts)), float(max(ts))],
                     "instances": [len(o["instances"]) if "instances" in o else 0 for o in outs]}
        if zoom is not None:
            e2e[name]["reports"] = [o["zoom_report"].tolist() for o in outs]
        pred.model.close()
    res["end_to_end"] = dict(e2e, frames=fb)
    return res


def report(paths):
    lines = lambda p: [json.loads(l) for l in open(p).read().strip().splitlines() if l.startswith("{")]
    T = lines(paths[0])[-1]
    f = lambda m: f"{m[0]:.3f} ({m[1]:.3f} .. {m[2]:.3f})"
    c = T["case"]
    out = ["# Zoom-in refinement on the device: the three entries per call, the numpy contract on the host, and a zoomed `predict_batch`", "",
           f"One MI355X (torch device name: {T['device']}); `tools/zoom_ab.py`, one session on one box.  Batch {c['batch']} at {c['width']}x{c['height']}, "
           f"{c['instances']} seeded instances per frame (rectangles and ellipses painted over each other), crop {c['crop']}: {c['batch'] * c['instances']} "
           f"crops per call; a context without a network.  Device milliseconds per call: HIP events around blocks of {T['calls']} calls, median "
           f"(min .. max) of {T['blocks']} blocks after {T['warmup']} block(s) of warm-up; every call reads the same input (calls rotating over "
           f"several inputs: not measured).  "
           f"The paste reads a stand-in for the crop pass's ids (`fake_crop_pass` of tests/test_zoom_cpu.py).  Host column: the numpy contract on "
           f"ONE frame of the same input on the same box.", "",
           "| entry | device, ms per call | device, ms per frame | host contract, s per frame | contract equal to the device's result |", "|---|---|---|---|---|"]
    for k in ("zoom_rois", "zoom_crop", "zoom_paste"):
        out.append(f"| {k} | {f(T['ms'][k])} | {T['ms'][k][0] / c['batch']:.4f} | {T['host_frame_s'][k]:.3f} | {'yes' if T['host_equal'] else 'NO'} |")
    r = T["report_mean"]
    out += ["", f"Per frame of that call (mean): {r[0]:.1f} crops, {r[1]:.1f} kept crop-pass instances, {r[2]:.1f} of them without a final id, {r[3]:.1f} final "
            f"instances.  The workspace the first call adds to the context: {T['workspace_bytes'] / 2 ** 20:.1f} MiB.", "",
            "Per kernel inside an entry: not measured.  Other batch sizes, frame sizes, instance counts and crop sizes: not measured.", ""]
    e = T["end_to_end"]
    out += [f"End to end, `predict_batch` of {e['frames']} seeded frames at {c['width']}x{c['height']} with 8 initial masks each, loud seeded weights, host "
            f"wall-clock milliseconds per call including the uploads and the result dicts, median (min .. max) of 5 calls after 2: plain "
            f"{f(e['plain']['ms'])}, `zoom=ZoomIn(crop={c['crop']})` {f(e['zoom']['ms'])} - {e['zoom']['ms'][0] / e['plain']['ms'][0]:.2f} x the plain call.  First-pass "
            f"instances per frame: {e['plain']['instances']}; zoom reports (crops, kept, without a final id, final): {e['zoom']['reports']}.  The {sum(e['plain']['instances'])} crops of {c['crop']}x{c['crop']} are {sum(e['plain']['instances']) * c['crop'] ** 2 / (c['width'] * c['height']):.0f} frames' worth of pixels against the "
            f"{e['frames']} frames of the plain call, and they run as {-(-sum(e['plain']['instances']) // 16)} calls of at most 16 crops.  The crop pass's forward time alone and the split of the zoomed call into its stages: not measured.  Batch 16 end to end: not measured.", ""]
    if len(paths) > 1:
        out += ["Plain `python bench.py --gpus 1 --steps 20 --warmup 5 --cpu-frames 0` (the feature is off there: no new kernel runs), this commit and its "
                "parent alternated in one session on one box:", "", "| run | commit | value | unit |", "|---|---|---|---|"]
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
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed block (one event pair per block)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--report", nargs="+", metavar="JSON")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    print(json.dumps(run(a)))


if __name__ == "__main__":
    main()
