"""GPU: iterative refinement (INTEGRATION.md "Iterative refinement"; csrc/iterate.hip).

The three kernels against the numpy contract of tests/test_iterate_cpu.py, exactly; the device loop against the same passes chained
through the host, bit for bit; every pass of the loop against the oracle on the loop's own input of that pass; convergence on weights
whose refinement is a fixed point by construction; the attribution of refined instances to the caller's masks; the adapter.
Loud heads (tests/test_gpu_loud_parity.py): real instances in every pass."""
import numpy as np
import pytest
import torch

from quber_amd import _lib, engine, synth
from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
from test_gpu_loud_parity import _check_heads, _oracle, _scene, loud_state_dict
from test_gpu_tta import HEADS, _check_post
from test_iterate_cpu import (TOP_K, fixed_point_state_dict, match_initial_np, oracle_pass, overlap_ids_np, overlap_masks_np,
                              relabel_np, same_segmentation_np)

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _engine(h, w, batch, n_masks=1):
    return engine.Engine(engine.make_config(h, w, max_batch=batch, max_instances=max(n_masks, 1), with_network=False), "cuda:0")


def _blocky(rng, shape, values, cell=7, noise=0.02):
    """An array of `shape` [B,H,W] drawn from `values`: constant cells of `cell` x `cell` pixels (runs, as label maps have them) with
    a sprinkle of single pixels."""
    B, H, W = shape
    coarse = rng.integers(0, len(values), (B, -(-H // cell), -(-W // cell)))
    idx = np.kron(coarse, np.ones((1, cell, cell), np.int64))[:, :H, :W]
    flip = rng.random(shape) < noise
    idx[flip] = rng.integers(0, len(values), int(flip.sum()))
    return np.asarray(values)[idx]


def _guarded(shape, dtype, shift):
    """A device tensor `shift` bytes into a byte buffer filled with 0x3C, and the buffer (guard bytes on both sides)."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((shift + n + 64,), 0x3C, dtype=torch.uint8, device="cuda")
    return buf, buf[shift:shift + n].view(dtype).view(shape), n


def _guards_intact(buf, shift, n):
    return bool((buf[:shift] == 0x3C).all()) and bool((buf[shift + n:] == 0x3C).all())


# ---- 1. relabel_panoptic ----
@pytest.mark.parametrize("h,w,counts,shift", [(96, 128, [5], 0), (96, 128, [0, 200, 1], 4), (75, 101, [1, 200], 4), (75, 101, [17, 0, 200], 12),
                                              (480, 640, [200, 23], 4), (64, 80, [500, 3], 0)],
                         ids=["96x128-b1", "96x128-b3", "75x101-b2", "75x101-b3", "640x480-b2", "count-above-top_k"])
@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
def test_relabel_panoptic_equals_contract(h, w, counts, shift, mirror):
    B = len(counts)
    rng = np.random.default_rng(h * w + sum(counts) + shift)
    labels = np.zeros((B, TOP_K), np.float32)
    pan = np.zeros((B, h, w), np.float32)
    for b, c in enumerate(counts):
        pool = np.arange(1000 if b % 2 == 0 else 1001, 1000 + 3 * TOP_K)         # a list holding 1000 in every other frame
        lst = np.sort(np.concatenate([pool[:1], rng.choice(pool[1:], TOP_K - 1, replace=False)])).astype(np.float32)   # not consecutive
        labels[b, :c] = lst[:c]
        labels[b, c:] = lst[c:][::-1]                                            # garbage behind count: must not match
        values = np.concatenate([lst[:c], lst[c:c + 3], [-1.0, -1.0, 0.0, 999.0, 1000.5, 70000.0]]).astype(np.float32)
        pan[b] = _blocky(rng, (1, h, w), values)[0]
    eng = _engine(h, w, 2 * B)
    post = {"panoptic": dev(pan), "labels": dev(labels), "count": dev(np.asarray(counts, np.int32))}
    fr = 2 * B if mirror else B
    buf, out, n = _guarded((fr, h, w), torch.int32, shift)                       # shift 4 / 12: a 4-byte-only alignment
    assert out.data_ptr() % 16 == shift % 16
    got = eng.relabel_panoptic(post, mirror=mirror, out=out)
    want = relabel_np(pan, labels, counts, mirror=mirror)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert _guards_intact(buf, shift, n)
    assert (want == 0).any() and (max(counts) == 0 or (want > 0).any()) and want.max() <= TOP_K
    np.testing.assert_array_equal(eng.relabel_panoptic(post, mirror=mirror).cpu().numpy(), want)      # a fresh, aligned output
    eng.close()


# ---- 2. overlap_masks ----
def _masks(rng, B, N, h, w):
    """Overlapping rectangles and speckle, inside = 1 / 7 / 255."""
    m = np.zeros((B, N, h, w), np.uint8)
    for b in range(B):
        for n in range(N):
            if n % 9 == 8:
                continue                                 # an empty mask
            y0, x0 = int(rng.integers(0, h - 1)), int(rng.integers(0, w - 1))
            y1, x1 = int(rng.integers(y0 + 1, h + 1)), int(rng.integers(x0 + 1, w + 1))
            m[b, n, y0:y1, x0:x1] = (1, 7, 255)[n % 3]
            if n % 4 == 0:
                m[b, n] |= (rng.random((h, w)) < 0.03).astype(np.uint8) * 7
    return m


@pytest.mark.parametrize("h,w,B,N,n_ids,shift,stray,cell", [
    (96, 128, 2, 200, 200, 0, False, 11), (96, 128, 1, 37, 254, 0, True, 11), (75, 101, 3, 37, 200, 0, False, 11), (96, 128, 2, 37, 1, 7, True, 11),
    (64, 80, 2, 1, 0, 0, True, 11), (64, 80, 3, 0, 200, 0, False, 11), (480, 640, 2, 37, 200, 0, False, 11),
    # an id map without runs: far more distinct (mask, id) cells per block than the block's table holds
    (96, 128, 1, 200, 254, 0, False, 1), (75, 101, 1, 37, 254, 0, False, 1)],
    ids=["n200", "ids254-stray", "75x101", "off7-ids1", "n1-ids0", "n0", "640x480", "no-runs", "75x101-no-runs"])
def test_overlap_masks_equals_contract(h, w, B, N, n_ids, shift, stray, cell):
    rng = np.random.default_rng(h * w + N + n_ids)
    values = list(range(0, n_ids + 1)) if n_ids < 12 or cell == 1 else [0, 0, 0] + list(rng.choice(np.arange(1, n_ids + 1), 9, replace=False)) + [n_ids]
    if stray:
        values += [-1, n_ids + 1, 255, 256, 70000, -2 ** 31]                   # outside 0..n_ids: counted nowhere
    ids = _blocky(rng, (B, h, w), np.asarray(values, np.int64), cell=cell).astype(np.int32)
    masks = _masks(rng, B, N, h, w)
    eng = _engine(h, w, B, N)
    buf, d_masks, n = _guarded((B, N, h, w), torch.uint8, shift)
    d_masks.copy_(dev(masks))
    table, area = eng.overlap_masks(d_masks, dev(ids), n_ids)
    t_np, a_np = overlap_masks_np(masks, ids, n_ids)
    assert table.shape == (B, N, n_ids + 1) and area.shape == (B, n_ids + 1)
    np.testing.assert_array_equal(table.cpu().numpy(), t_np)
    np.testing.assert_array_equal(area.cpu().numpy(), a_np)
    if not stray:
        np.testing.assert_array_equal(t_np.sum(2), (masks != 0).sum((2, 3)))    # every row sums to the mask's pixel count
        assert (a_np.sum(1) == h * w).all()
    # a second call into the same buffers overwrites, it does not accumulate
    eng.overlap_masks(d_masks, dev(ids), n_ids, out=(table, area))
    np.testing.assert_array_equal(table.cpu().numpy(), t_np)
    np.testing.assert_array_equal(area.cpu().numpy(), a_np)
    if N:                                                # the area is optional in the C ABI
        t2 = torch.full_like(table, 77)
        _lib.check(eng.lib.quber_overlap_masks(eng.h, engine._ptr(d_masks), engine._ptr(dev(ids)), B, N, n_ids, engine._ptr(t2), None,
                                               engine._stream()))
        np.testing.assert_array_equal(t2.cpu().numpy(), t_np)
    assert _guards_intact(buf, shift, n)
    eng.close()


# ---- 3. overlap_ids ----
@pytest.mark.parametrize("h,w,B,n_a,n_b,stray,runs", [(96, 128, 2, 200, 200, False, True), (75, 101, 3, 254, 1, True, True), (64, 80, 1, 0, 0, True, True),
                                                      (75, 101, 2, 1, 254, False, True), (480, 640, 2, 200, 200, False, True),
                                                      (96, 128, 2, 254, 254, False, False)],
                         ids=["200x200", "75x101-254x1-stray", "0x0", "75x101-1x254", "640x480", "no-runs"])
def test_overlap_ids_equals_contract(h, w, B, n_a, n_b, stray, runs):
    rng = np.random.default_rng(h + w + n_a + 3 * n_b)

    def ids_for(n, cell):
        values = list(range(0, n + 1)) if n < 12 or not runs else [0, 0] + list(rng.choice(np.arange(1, n + 1), 10, replace=False)) + [n]
        if stray:
            values += [-1, n + 1, 70000]
        return _blocky(rng, (B, h, w), np.asarray(values, np.int64), cell=cell if runs else 1).astype(np.int32)

    a, b = ids_for(n_a, 9), ids_for(n_b, 13)
    eng = _engine(h, w, B)
    buf_a, d_a, n = _guarded((B, h, w), torch.int32, 4)                          # 4-byte-only alignment on one side
    d_a.copy_(dev(a))
    want = overlap_ids_np(a, b, n_a, n_b)
    table = eng.overlap_ids(d_a, dev(b), n_a, n_b)
    np.testing.assert_array_equal(table.cpu().numpy(), want)
    if not stray:
        assert (want.sum((1, 2)) == h * w).all()
    eng.overlap_ids(d_a, dev(b), n_a, n_b, out=table)
    np.testing.assert_array_equal(table.cpu().numpy(), want)
    eng.close()


# ---- scenes and weights of the loop tests ----
_CASE = {}


def _case(h, w, b, n):
    key = (h, w, b, n)
    if key not in _CASE:
        batch, offs, image = _scene(11, b, h, w, n)
        sd1 = _CASE.get((h, w, 1, n))
        sd = sd1[1] if sd1 is not None else loud_state_dict(2, image[:1], offs[:1], n)
        _CASE[key] = (batch, sd, image)
    return _CASE[key]


def _set_mode(monkeypatch, mode):
    """Every engine the predictors build from here on computes in quber_config.compute_dtype = mode."""
    orig = engine.make_config

    def make_config(*a, **kw):
        qc = orig(*a, **kw)
        qc.compute_dtype = mode
        return qc
    monkeypatch.setattr(engine, "make_config", make_config)


def _feedback(out, h, w):
    """What a caller feeds back through the host: the refined masks as uint8 * 255 (an empty list when there are no instances)."""
    if "instances" not in out:
        return np.zeros((0, h, w), np.uint8)
    return out["instances"].pred_masks.cpu().numpy().astype(np.uint8) * 255


def _same_outputs(got, want, what):
    for key in ("sem_seg", "eee_boundary"):
        assert torch.equal(got[key], want[key]), (what, key)
    assert torch.equal(got["panoptic_seg"][0], want["panoptic_seg"][0]), what
    assert ("instances" in got) == ("instances" in want), what
    if "instances" in got:
        gi, wi = got["instances"], want["instances"]
        assert torch.equal(gi.pred_masks, wi.pred_masks) and torch.equal(gi.pred_boxes.tensor, wi.pred_boxes.tensor), what
        assert torch.equal(gi.pred_classes, wi.pred_classes), what
        # post_paint_stats sums the foreground probabilities with float64 atomic adds: their order can move the last bit
        np.testing.assert_allclose(gi.scores.cpu().numpy(), wi.scores.cpu().numpy(), rtol=2e-5, atol=1e-6)


def _k(out):
    return len(out["instances"]) if "instances" in out else 0


# ---- 4. the loop equals the chain, bit for bit ----
@pytest.mark.parametrize("h,w,n,ks", [(192, 256, 6, (2, 3)), (480, 640, 8, (2,))], ids=["256x192", "640x480"])
@pytest.mark.parametrize("mode", [0, 3], ids=["f32", "bf16x3"])
def test_predict_loop_equals_host_chain(h, w, n, ks, mode, monkeypatch):
    _set_mode(monkeypatch, mode)
    batch, sd, _ = _case(h, w, 1, n)
    rgb, dep, masks = batch["rgb"][0], batch["depth"][0], batch["masks"][0]
    one = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd)
    chain, m = [], masks
    for p in range(max(ks)):
        out = one.predict(rgb, dep, m)[0]
        assert _k(out) >= 1, f"pass {p + 1} of the chain has no instance"
        assert "refine_passes" not in out and "initial_overlap" not in out
        chain.append(out)
        m = _feedback(out, h, w)
    one.model.close()
    for k in ks:
        pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, iterations=k)
        out = pred.predict(rgb, dep, masks)[0]
        assert out["refine_passes"] == k and 0 <= out["refine_converged_at"] <= k
        _same_outputs(out, chain[k - 1], f"iterations={k}")
        assert pred.model.engine_for(h, w, 1).qcfg.max_instances >= TOP_K
        pred.model.close()
    assert not torch.equal(chain[0]["panoptic_seg"][0], chain[1]["panoptic_seg"][0]), "the second pass changes nothing: the comparison is blind"


def test_batch_stream_and_tta_loops_equal_host_chain():
    h, w, n = 192, 256, 6
    batch, sd, _ = _case(h, w, 3, n)
    rgb, dep = batch["rgb"], batch["depth"]
    masks = [batch["masks"][0], batch["masks"][1][:4], batch["masks"][2][:2]]   # different mask counts
    # predict_batch
    one = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd)
    first = one.predict_batch(rgb, dep, masks)
    assert all(_k(o) >= 1 for o in first)
    want = one.predict_batch(rgb, dep, [_feedback(o, h, w) for o in first])
    assert all(_k(o) >= 1 for o in want)
    two = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, iterations=2)
    got = two.predict_batch(rgb, dep, masks)
    for b in range(3):
        assert got[b]["refine_passes"] == 2
        _same_outputs(got[b], want[b], f"predict_batch frame {b}")

    # enqueue_batch / collect_batch on the same frames
    def stream(pred, mk):
        nn = max([len(x) for x in mk] + [1])
        pad = np.zeros((3, nn, h, w), np.uint8)
        for b, x in enumerate(mk):
            pad[b, :len(x)] = x
        hd = pred.model.enqueue_batch(dev(rgb), dev(dep), dev(pad))
        return pred.model.collect_batch(hd)[0]
    s1 = stream(one, masks)
    s_want = stream(one, [_feedback(o, h, w) for o in s1])
    s_got = stream(two, masks)
    for b in range(3):
        assert s_got[b]["refine_passes"] == 2 and _k(s_want[b]) >= 1
        _same_outputs(s_got[b], s_want[b], f"stream frame {b}")
    one.model.close()
    two.model.close()
    # test-time augmentation, batch 1: every pass is an augmented pass
    t1 = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, tta=True)
    a = t1.predict(rgb[0], dep[0], masks[0])[0]
    b2 = t1.predict(rgb[0], dep[0], _feedback(a, h, w))[0]
    sb = t1.predict_batch(rgb[:1], dep[:1], [_feedback(t1.predict_batch(rgb[:1], dep[:1], masks[:1])[0], h, w)])[0]
    t1.model.close()
    t2 = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, tta=True, iterations=2)
    assert _k(a) >= 1 and _k(b2) >= 1
    _same_outputs(t2.predict(rgb[0], dep[0], masks[0])[0], b2, "tta predict")
    _same_outputs(t2.predict_batch(rgb[:1], dep[:1], masks[:1])[0], sb, "tta predict_batch")
    t2.model.close()


# ---- 5. against the oracle, pass by pass, teacher-forced ----
def test_every_pass_against_the_oracle_on_its_own_input():
    """A free-running CPU chain cannot be compared over several passes (a 1e-5 logit difference flips a near-tie pixel and the next
    pass starts from another mask), so every pass of the device loop is held to the oracle on the loop's OWN input of that pass."""
    h, w, n, k = 192, 256, 6, 3
    batch, sd, image = _case(h, w, 1, n)
    pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, iterations=k)
    pred.model.debug_passes = rec = []
    out = pred.predict(batch["rgb"][0], batch["depth"][0], batch["masks"][0])[0]
    assert len(rec) == k and out["refine_passes"] == k
    net = _oracle(sd)
    eng = pred.model.engine_for(h, w, 1)
    for p, r in enumerate(rec):
        if p == 0:
            masks = batch["masks"][0]
        else:
            ids = r["ids_in"][0].cpu().numpy()
            assert np.array_equal(ids, rec[p - 1]["ids_out"][0].cpu().numpy())
            masks = np.stack([(ids == j).astype(np.uint8) for j in range(1, int(ids.max()) + 1)])
        ref, _ = oracle_pass(net, image, masks)
        logits = r["logits"].cpu()
        _check_heads(logits, ref, HEADS)
        post = {key: v.cpu() for key, v in r["post"].items()}
        kk = int(post["count"][0])
        assert kk >= 1, f"pass {p + 1} has no instance"
        pm = eng.extract_masks(r["post"], kk).cpu().numpy()
        assert _check_post(logits, post, pm) == [kk]
        np.testing.assert_array_equal(r["ids_out"].cpu().numpy(), relabel_np(post["panoptic"].numpy(), post["labels"].numpy(), [kk]))
    assert torch.equal(out["sem_seg"], rec[-1]["logits"][0, 0:1]) and torch.equal(out["panoptic_seg"][0], rec[-1]["post"]["panoptic"][0])
    # refine_converged_at is whatever the device flags say: the contract evaluated on the kept ids
    maps = [r["ids_out"].cpu().numpy() for r in rec]
    same = [same_segmentation_np(overlap_ids_np(maps[p - 1], maps[p], TOP_K, TOP_K)[0]) for p in range(1, k)]
    assert out["refine_converged_at"] == (same.index(True) + 2 if True in same else 0)
    pred.model.close()


# ---- 6. convergence ----
def test_until_converged_stops_at_the_fixed_point():
    h, w = 96, 128
    batch, _, _ = _scene(5, 1, h, w, 3)
    rgb, dep, masks = batch["rgb"][0], batch["depth"][0], batch["masks"][0]
    sd = fixed_point_state_dict()
    outs = {}
    for name, kw in (("stop", dict(iterations=5, until_converged=True)), ("two", dict(iterations=2)), ("five", dict(iterations=5))):
        pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, **kw)
        outs[name] = pred.predict(rgb, dep, masks)[0]
        if name == "stop":
            outs["stop_batch"] = pred.predict_batch(rgb[None], dep[None], [masks])[0]
            hd = pred.model.enqueue_batch(dev(rgb[None]), dev(dep[None]), dev(masks[None]))
            outs["stop_stream"] = pred.model.collect_batch(hd)[0][0]                  # the stream always runs the fixed count
        pred.model.close()
    assert (outs["stop"]["refine_passes"], outs["stop"]["refine_converged_at"]) == (2, 2)
    assert (outs["stop_batch"]["refine_passes"], outs["stop_batch"]["refine_converged_at"]) == (2, 2)
    assert (outs["stop_stream"]["refine_passes"], outs["stop_stream"]["refine_converged_at"]) == (5, 2)
    assert (outs["two"]["refine_passes"], outs["two"]["refine_converged_at"]) == (2, 2)
    assert (outs["five"]["refine_passes"], outs["five"]["refine_converged_at"]) == (5, 2)
    for name in ("two", "five", "stop_batch", "stop_stream"):
        for key in ("sem_seg", "eee_boundary"):
            assert torch.equal(outs["stop"][key], outs[name][key]), (name, key)
        assert torch.equal(outs["stop"]["panoptic_seg"][0], outs[name]["panoptic_seg"][0]), name
    assert _k(outs["stop"]) == 1 and bool(outs["stop"]["instances"].pred_masks.all())
    assert float(outs["stop"]["panoptic_seg"][0].min()) == 1000.0


def test_decode_errors_decodes_the_last_pass_and_leaves_mask_hist_out():
    h, w, n = 192, 256, 6
    batch, sd, _ = _case(h, w, 1, n)
    args = (batch["rgb"][0], batch["depth"][0], batch["masks"][0])
    pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, iterations=2, decode_errors=True)
    outs = [pred.predict(*args)[0], pred.predict_batch(args[0][None], args[1][None], [args[2]])[0]]
    hd = pred.model.enqueue_batch(dev(args[0][None]), dev(args[1][None]), dev(args[2][None]))
    outs.append(pred.model.collect_batch(hd)[0][0])
    pred.model.close()
    for out in outs:
        assert out["refine_passes"] == 2 and "eee_boundary_mask_hist" not in out
        assert torch.equal(out["eee_boundary_classes"], torch.argmax(out["eee_boundary"], 0).to(torch.uint8))
        assert int(out["eee_boundary_hist"].sum()) == h * w
    one = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, decode_errors=True)
    assert "eee_boundary_mask_hist" in one.predict(*args)[0]                     # one pass: as before
    one.model.close()


# ---- 7. track_initial ----
def _check_tracking(out, masks, h, w):
    pan = out["panoptic_seg"][0].cpu().numpy()
    k = _k(out)
    lst = np.unique(pan[pan != -1])
    assert len(lst) == k
    labels = np.zeros((1, TOP_K), np.float32)
    labels[0, :k] = lst
    ids = relabel_np(pan[None], labels, [k])
    table, area = overlap_masks_np(np.asarray(masks)[None].reshape(1, len(masks), h, w), ids, k)
    ov, index, iou = match_initial_np(table[0], area[0])
    got = out["initial_overlap"]
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(masks), k + 1)
    np.testing.assert_array_equal(got.cpu().numpy(), ov)
    if k:
        inst = out["instances"]
        assert inst.initial_index.dtype == torch.int64 and inst.initial_iou.dtype == torch.float32
        np.testing.assert_array_equal(inst.initial_index.cpu().numpy(), index)
        np.testing.assert_array_equal(inst.initial_iou.cpu().numpy().view(np.uint32), iou.view(np.uint32))
    return index


@pytest.mark.parametrize("iterations", [1, 2])
def test_track_initial_equals_contract(iterations):
    h, w, n = 192, 256, 6
    batch, sd, _ = _case(h, w, 3, n)
    rgb, dep = batch["rgb"], batch["depth"]
    masks = [batch["masks"][0], np.zeros((0, h, w), np.uint8), batch["masks"][2][:3]]      # different N_b, one frame without masks
    pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, iterations=iterations, track_initial=True)
    out = pred.predict(rgb[0], dep[0], masks[0])[0]
    index = _check_tracking(out, masks[0], h, w)
    assert _k(out) >= 1 and (index >= 0).any()
    outs = pred.predict_batch(rgb, dep, masks)
    for b in range(3):
        _check_tracking(outs[b], masks[b], h, w)
    pad = np.zeros((3, n, h, w), np.uint8)
    for b, x in enumerate(masks):
        pad[b, :len(x)] = x
    hd = pred.model.enqueue_batch(dev(rgb), dev(dep), dev(pad), n_masks=[len(x) for x in masks])
    for b, o in enumerate(pred.model.collect_batch(hd)[0]):
        _check_tracking(o, masks[b], h, w)
    hd = pred.model.enqueue_batch(dev(rgb), dev(dep), dev(pad))                            # counts not given: all N rows
    for b, o in enumerate(pred.model.collect_batch(hd)[0]):
        _check_tracking(o, pad[b], h, w)
    pred.model.close()
    if iterations == 1:                                  # the rest of the dict is what a predictor without the flag returns
        plain = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd)
        want = plain.predict(rgb[0], dep[0], masks[0])[0]
        assert set(out) - set(want) == {"initial_overlap"} and set(want) <= set(out)
        _same_outputs(out, want, "track_initial, iterations=1")
        assert set(out["instances"].get_fields()) - set(want["instances"].get_fields()) == {"initial_index", "initial_iou"}
        plain.model.close()


# ---- 8. the adapter ----
def test_adapter_predict_and_stream_with_iterations(tmp_path):
    """MaskRefiner(iterations=2) on files: predict against predict_stream(batch=2).  The second pass starts from masks that may differ
    in a few near-tie pixels between a batch-1 and a batch-2 run; measured, the two-pass distances sit at the single-pass
    batch-invariance level (1.3e-5 on sem_seg, every label-map pixel equal: profiles/iterate_ab.md), so the bars are the single-pass
    ones, 1e-4 / 0.9999 (profiles/r20_batch_invariance.txt).  A wrong feedback moves whole instances."""
    from PIL import Image
    from quber_amd.eval.refiner_model import MaskRefiner
    h, w, n = 480, 640, 8
    batch, sd, _ = _case(h, w, 1, n)
    scenes = [synth.make_scene(60 + i, h, w, n) for i in range(2)]
    rgb = np.stack([batch["rgb"][0]] + [s["rgb"] for s in scenes])
    dep = np.stack([batch["depth"][0]] + [s["depth"] for s in scenes])
    masks = [batch["masks"][0]] + [s["masks"] for s in scenes]
    items = []
    for i in range(3):
        Image.fromarray(rgb[i][:, :, ::-1].copy()).save(tmp_path / f"rgb{i}.png")
        Image.fromarray(dep[i][:, :, 0].astype(np.uint16) * 5 + 300).save(tmp_path / f"depth{i}.png")
        items.append((str(tmp_path / f"rgb{i}.png"), str(tmp_path / f"depth{i}.png"), masks[i] != 0, None))
    ref = MaskRefiner(None, weights_file=None, dataset="OSD", iterations=2)
    assert ref.refiner_predictor.iterations == 2 and ref.refiner_predictor.model.iterations == 2
    ref.refiner_predictor.model.state_dict = sd
    ref.refiner_predictor.model._engines.clear()
    seq = [ref.predict(*it) for it in items]
    got = list(ref.predict_stream(items, workers=2, batch=2))
    assert len(got) == 3 and sum(len(r[0]) for r in seq) >= 1
    for i, ((m0, o0, _, _), (m1, o1, _, _)) in enumerate(zip(seq, got)):
        assert o0["refine_passes"] == 2 and o1["refine_passes"] == 2
        d = float((o0["sem_seg"] - o1["sem_seg"]).abs().max())
        eq = float((o0["panoptic_seg"][0] == o1["panoptic_seg"][0]).float().mean())
        print(f"adapter iterations=2 frame {i}: max |sem_seg batch 1 - batch 2| = {d:.3e}, equal label-map pixels = {eq:.6f}, "
              f"instances {_k(o0)} / {_k(o1)}")
        assert _k(o0) == _k(o1) and len(m0) == len(m1)
        assert d < 1e-4 and eq > 0.9999
    ref.refiner_predictor.model.close()
