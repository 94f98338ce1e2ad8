"""Child process of tests/test_gpu_error_decode.py::test_error_chain_graph_replay_equals_eager: error_decode -> error_mask_hist ->
error_score captured as one hipGraph (a straight chain on one stream, no parallel branches) and replayed twice, against the eager
results and the numpy statements.  Every buffer is allocated before the capture; the graph is destroyed before the engine.  Prints
one JSON line."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from quber_amd import engine, synth  # noqa: E402
from test_error_decode_cpu import confusion_np, decode_np, mask_hist_np  # noqa: E402


def main():
    h, w, b, n = 96, 128, 2, 5
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    eng = engine.Engine(engine.make_config(h, w, max_batch=b, max_instances=8, with_network=False), dev)
    init = np.stack([(synth.make_scene(s, h, w, n)["masks"] != 0).astype(np.uint8) for s in (1, 2)])
    gt = np.stack([(synth.make_scene(s, h, w, n)["masks"] != 0).astype(np.uint8) for s in (5, 6)])
    d_init, d_gt = torch.from_numpy(init).to(dev), torch.from_numpy(gt).to(dev)
    logits = torch.from_numpy(rng.integers(-2, 3, (b, 8, h, w)).astype(np.float32)).to(dev)      # ties everywhere
    explicit = eng.error_maps(d_init, d_gt)
    cls = torch.empty((b, h, w), dtype=torch.uint8, device=dev)
    hist = torch.empty((b, 4), dtype=torch.int32, device=dev)
    mh = torch.empty((b, n, 4), dtype=torch.int32, device=dev)
    table = torch.empty((b, 5, 4), dtype=torch.int64, device=dev)
    outs = (cls, hist, mh, table)

    def step():
        eng.error_decode(logits, (4, 4), cls, hist)
        eng.error_mask_hist(cls, d_init, 4, mh)
        eng.error_score(cls, explicit, 1, "e3", table)

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
    eager = [t.clone() for t in outs]
    c_np, h_np = decode_np(logits.cpu().numpy(), 4, 4)
    ok_np = bool(np.array_equal(eager[0].cpu().numpy(), c_np) and np.array_equal(eager[1].cpu().numpy(), h_np)
                 and np.array_equal(eager[2].cpu().numpy(), mask_hist_np(c_np, init, 4))
                 and np.array_equal(eager[3].cpu().numpy(), confusion_np(c_np, explicit.cpu().numpy(), 1, "e3")))
    same = []
    for _ in range(2):
        for t in outs:
            t.fill_(77)                                  # whatever the buffers hold, a replay overwrites it
        graph.replay()
        torch.cuda.synchronize()
        same.append(all(bool(torch.equal(t, e)) for t, e in zip(outs, eager)))
    # a replay on top of the previous replay's results (nothing cleared in between): the counters do not accumulate
    graph.replay()
    torch.cuda.synchronize()
    same[1] = same[1] and all(bool(torch.equal(t, e)) for t, e in zip(outs, eager))
    res = {"eager_equals_numpy": ok_np, "replay_equals_eager": same[0], "second_replay_equals_eager": same[1],
           "pixels": int(eager[2].sum())}
    del graph                                            # the graph before the engine
    torch.cuda.synchronize()
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
