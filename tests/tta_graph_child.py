"""Child process of tests/test_gpu_tta.py::test_tta_step_graph_replay_equals_eager: the TTA step (flip -> encode -> forward of 2
frames -> merge -> post-processing) captured as one hipGraph at B = 1 and replayed, against the eager step.  Every buffer is allocated
before the capture; the graph is destroyed before the engine.  Prints one JSON line."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from quber_amd import arch, engine, synth  # noqa: E402
from quber_amd.maskrefiner.predictor import RefinerModel  # noqa: E402


def main():
    h, w, n = 192, 256, 6
    dev = "cuda:0"
    batch = synth.make_batch(11, 1, h, w, n)

    def two(a):
        t = torch.full((2 * a.shape[0],) + a.shape[1:], 0xA5, dtype=torch.uint8, device=dev)
        t[:a.shape[0]].copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return t

    bgr2, dep2, m2 = two(batch["rgb"]), two(batch["depth"]), two(batch["masks"])
    # loud heads, centre bias calibrated on the HIP path's own centre logits of the frame (as __graft_entry__.smoke does)
    eng0 = engine.Engine(engine.make_config(h, w, max_batch=2, max_instances=n), dev)
    eng0.load_state_dict(arch.init_state_dict(seed=2, loud_heads=True))
    c0 = eng0.forward(bgr2[:1].contiguous(), dep2[:1].contiguous(), eng0.encode(m2[:1].contiguous()))[:, 1:2].float().cpu()
    eng0.close()
    sd = arch.init_state_dict(seed=2, loud_heads=True, center_bias=arch.calibrate_center_bias(c0, n))
    eng = engine.Engine(engine.make_config(h, w, max_batch=2, max_instances=n), dev)
    eng.load_state_dict(sd)
    offsets = torch.empty((2, 3, h, w), dtype=torch.float32, device=dev)
    logits2 = torch.empty((2, eng.planes, h, w), dtype=torch.float32, device=dev)
    merged = torch.empty((1, eng.planes, h, w), dtype=torch.float32, device=dev)
    post = eng.alloc_post(1)

    def step():
        eng.tta_flip_inputs(bgr2, dep2, m2)
        eng.encode(m2, offsets)
        eng.forward(bgr2, dep2, offsets, logits2)
        eng.tta_merge(logits2, merged)
        eng.postprocess(merged, post)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    step()                                               # eager, same inputs
    torch.cuda.synchronize()
    eager = (merged.clone(), post["panoptic"].clone(), post["count"].clone(), bgr2[1:].clone(), dep2[1:].clone(), m2[1:].clone())
    ref = RefinerModel(None, sd, dev, tta=True).tta_logits(eng, bgr2, dep2, m2)      # the predictor's step, eager
    torch.cuda.synchronize()
    same_step = bool(torch.equal(ref, eager[0]))
    for t in (merged, post["panoptic"], bgr2[1:], dep2[1:], m2[1:]):
        t.zero_()
    graph.replay()
    graph.replay()                                       # steady state: replays are idempotent
    torch.cuda.synchronize()
    res = {"flip_in_graph": bool(torch.equal(bgr2[1:], eager[3]) and torch.equal(dep2[1:], eager[4]) and torch.equal(m2[1:], eager[5])),
           "step_is_tta_logits": same_step,
           "replay_equals_eager": bool(torch.equal(merged, eager[0]) and torch.equal(post["panoptic"], eager[1])
                                       and torch.equal(post["count"], eager[2])),
           "instances": int(post["count"][0])}
    del graph                                            # the graph before the engine whose streams and events it was captured on
    torch.cuda.synchronize()
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
