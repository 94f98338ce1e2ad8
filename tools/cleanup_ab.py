"""Connected-component clean-up on one MI355X: quber_cleanup_postprocess next to the quber_postprocess it follows.  Batch 16, 640x480,
head outputs of `synth` scenes (synth.fake_head_outputs: N = 20 objects per frame, Gaussian noise on the foreground logit and the
offsets so that specks and holes exist), a context without a network.  Prints ONE JSON line.

  --post-only    only calls that exist without the feature, so it also runs on a checkout of the parent commit (--root DIR: import
                 quber_amd from there): the stage profile of quber_postprocess on the same inputs
  default        this commit: the same, and per preset (Cleanup.uois(), Cleanup.sam(), both at once) the device time of
                 quber_cleanup_postprocess between two events and its stage profile (cleanup_label, cleanup_apply, iterate_relabel, zero)
  --label TEXT   kept in the line; with QUBER_LIB=<another build of the library> a variant of the kernels is timed on the same inputs
  --report PARENT.json THIS.json [MORE.json ...]   the markdown record (profiles/cleanup_ab.md).  Further files are told apart by what
                 they hold: lines of this tool (other noise levels, labelled variants) or the JSON result lines of plain `python bench.py`
                 runs of the two commits, alternated in one session

    python3 tools/cleanup_ab.py [--post-only] [--root DIR] [--noise 0.8] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

H, W, N, B = 480, 640, 20, 16


def setup(a):
    sys.path.insert(0, os.path.abspath(a.root) if a.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from oracle import encode_np
    from quber_amd import engine, synth
    frames = []
    for f in range(B):
        sc = synth.make_scene(900 + f, H, W, N)
        enc = encode_np.encode_initial_masks(sc["masks"])
        frames.append(np.concatenate(synth.fake_head_outputs(enc, sc["masks"], np.random.default_rng(950 + f), noise=a.noise)))
    logits = torch.from_numpy(np.stack(frames).astype(np.float32)).to("cuda:0")
    eng = engine.Engine(engine.make_config(H, W, max_batch=B, max_instances=N, with_network=False), "cuda:0")
    return torch, eng, logits


def profiled(eng, fn, before, steps, warmup):
    """-> {stage: dict(ms = median over the steps, launches, bytes)} of fn(); before() runs outside the bracket"""
    profs = []
    for i in range(warmup + steps):
        before()
        eng.profile_begin()
        fn()
        p = eng.profile_end()
        if i >= warmup:
            profs.append(p)
    return {k: {"ms": float(np.median([p[k]["ms"] for p in profs])), "launches": profs[0][k]["launches"], "bytes": profs[0][k]["bytes"]}
            for k in profs[0]}


def timed(torch, fn, before, steps, warmup):
    """-> (median, min, max) device milliseconds of fn() between two events; before() runs outside them"""
    ms = []
    for i in range(warmup + steps):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def run(a):
    torch, eng, logits = setup(a)
    post = eng.alloc_post(B)
    nothing = lambda: None
    res = {"mode": "post-only" if a.post_only else "cleanup", "noise": a.noise, "label": a.label, "device": torch.cuda.get_device_name(0)}
    res["postprocess_ms"] = timed(torch, lambda: eng.postprocess(logits, post), nothing, a.steps, a.warmup)
    res["postprocess_stages"] = profiled(eng, lambda: eng.postprocess(logits, post), nothing, a.steps, a.warmup)
    res["instances_per_frame_mean"] = float(post["count"].float().mean())
    if not a.post_only:
        from quber_amd.cleanup import Cleanup
        report = torch.empty((B, eng.cap + 1, 4), dtype=torch.int32, device="cuda:0")
        res["presets"] = {}
        for name, opts in (("off", Cleanup()), ("uois", Cleanup.uois()), ("sam", Cleanup.sam()), ("both", Cleanup(True, 4, 0, 300))):
            before = lambda: eng.postprocess(logits, post)
            fn = lambda: eng.cleanup_post(logits, post, opts, report)
            ms = timed(torch, fn, before, a.steps, a.warmup)
            stages = profiled(eng, fn, before, a.steps, a.warmup)
            rep = report.cpu().numpy().astype(np.int64)
            res["presets"][name] = {"ms": ms, "stages": stages, "components": int(rep[:, 1:, 0].sum()), "removed": int(rep[:, 1:, 1].sum()),
                                    "void_components": int(rep[:, 0, 0].sum()), "filled": int(rep[:, 0, 2].sum())}
    eng.close()
    return res


def report(paths):
    last = lambda p: json.loads([l for l in open(p).read().strip().splitlines() if l.startswith("{")][-1])
    P, T = last(paths[0]), last(paths[1])
    more = [(p, last(p)) for p in paths[2:]]
    runs = [("this", T)] + [(r.get("label") or os.path.basename(p), r) for p, r in more if r.get("mode") == "cleanup"]
    bench = [p for p, r in more if "mode" not in r]
    ssum = lambda st: sum(v["ms"] for v in st.values())
    f = lambda m: f"{m[0]:.4f} ({m[1]:.4f} .. {m[2]:.4f})"
    out = ["# Connected-component clean-up next to the post-processing it follows", "",
           f"One MI355X (torch device name: {T['device']}); batch {B}, {W}x{H}, head outputs of `synth` scenes (N = {N} objects, Gaussian noise on the foreground logit and the "
           "offsets), a context without a network; device milliseconds per batch between two events, median (min .. max) of 20 calls after 3; "
           "`tools/cleanup_ab.py`, every line taken in one session on one box.", "",
           "| what | build | noise | ms per batch |", "|---|---|---|---|",
           f"| `quber_postprocess` | parent | {P['noise']} | {f(P['postprocess_ms'])} |"]
    for who, R in runs:
        out.append(f"| `quber_postprocess` | {who} | {R['noise']} | {f(R['postprocess_ms'])} |")
    for who, R in runs:
        for name, r in R["presets"].items():
            out.append(f"| `quber_cleanup_postprocess`, {name} | {who} | {R['noise']} | {f(r['ms'])} |")
    out += ["", "Per run: instances per frame; per preset the components of the instances found / pixels removed / void components examined / "
            "pixels filled over the 16 frames:", ""]
    for who, R in runs:
        out.append(f"- {who}, noise {R['noise']}: {R['instances_per_frame_mean']:.1f} instances per frame; " +
                   "; ".join(f"{k}: {r['components']} / {r['removed']} / {r['void_components']} / {r['filled']}" for k, r in R["presets"].items()))
    out += ["", "Stages (stage profiler; every bracket is its own pair of events, so the sums exceed the event-to-event times by what the brackets add):", "",
            "| run | call | stage | launches | ms | algorithmic MB | GB/s |", "|---|---|---|---|---|---|---|"]
    for who, R in runs:
        rows = [("quber_postprocess", R["postprocess_stages"])] + [(f"cleanup, {k}", r["stages"]) for k, r in R["presets"].items()]
        for call, st in rows:
            for k, s in st.items():
                out.append(f"| {who}, noise {R['noise']} | {call} | {k} | {s['launches']} | {s['ms']:.4f} | {s['bytes'] * 1e-6:.1f} | {s['bytes'] / max(s['ms'], 1e-9) * 1e-6:.0f} |")
    if bench:
        out += ["", "Plain `python bench.py` (the feature is off there), the two builds alternated in one session:", "",
                "| file | masks/s | ms per step |", "|---|---|---|"]
        for p in bench:
            for line in open(p).read().strip().splitlines():
                if line.startswith("{"):
                    j = json.loads(line)
                    out.append(f"| {os.path.basename(p)} | {j.get('value')} | {j.get('ms_per_step')} |")
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--post-only", action="store_true")
    ap.add_argument("--root", default=None, help="import quber_amd from this checkout instead of the one this file lies in")
    ap.add_argument("--noise", type=float, default=0.8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="", help="kept in the JSON line (names a QUBER_LIB variant)")
    ap.add_argument("--report", nargs="+", metavar="JSON")
    a = ap.parse_args()
    if a.report:
        return report(a.report)
    print(json.dumps(run(a)))


if __name__ == "__main__":
    main()
