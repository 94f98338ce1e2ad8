"""GPU: horizontal-flip test-time augmentation (INTEGRATION.md "Test-time augmentation"; csrc/tta.hip).

The flip kernel against np.flip, the merge kernel against the numpy statement of tests/test_tta_cpu.py, the merged heads against
the same merge of the CPU oracle's outputs on x and flip(x), post-processing of the merged logits against oracle/postproc_ref.py,
flip equivariance, the single-stream config and the public API.  Loud heads (tests/test_gpu_loud_parity.py)."""
import numpy as np
import pytest
import torch

from oracle import encode_np, postproc_ref
from quber_amd import arch, engine, synth
from test_gpu_loud_parity import _check_heads, _oracle, _scene, loud_state_dict
from test_tta_cpu import X_OFFSET_PLANE, mirror_logits_np, tta_merge_np

pytestmark = pytest.mark.gpu

HEADS = ("foreground", "center", "offset", "eee_boundary")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def two(a):
    """[B,...] numpy -> [2B,...] device tensor with the frames in the first half (the second half is garbage)."""
    t = torch.full((2 * a.shape[0],) + a.shape[1:], 0xA5, dtype=torch.uint8, device="cuda")
    t[:a.shape[0]].copy_(dev(a))
    return t


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. flip kernel ----
@pytest.mark.parametrize("h,w,b,n,shift", [(96, 241, 1, 0, 0), (96, 241, 1, 37, 0), (64, 128, 2, 5, 0), (48, 97, 3, 4, 7)],
                         ids=["96x241-n0", "96x241-n37", "64x128-b2", "48x97-b3-unaligned"])
def test_flip_kernel_and_mirrored_encoding(h, w, b, n, shift):
    rng = np.random.default_rng(h * w + n)
    rgb = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    dep = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    masks = np.stack([synth.make_scene(s, h, w, n)["masks"] for s in range(b)]) if n else np.zeros((b, 0, h, w), np.uint8)
    eng = engine.Engine(engine.make_config(h, w, max_batch=2 * b, max_instances=max(n, 1), with_network=False), "cuda:0")

    def at(a):
        # the buffers `shift` bytes into an allocation: unaligned spans on both the load and the store side
        buf = torch.full((shift + 2 * a.size + 64,), 0x3C, dtype=torch.uint8, device="cuda")
        t = buf[shift:shift + 2 * a.size].view((2 * a.shape[0],) + a.shape[1:])
        t[:a.shape[0]].copy_(dev(a))
        return buf, t

    (bb, bgr2), (db, dep2), (mb, m2) = at(rgb), at(dep), at(masks)
    eng.tta_flip_inputs(bgr2, dep2, m2 if n else None)
    np.testing.assert_array_equal(bgr2[:b].cpu().numpy(), rgb)
    np.testing.assert_array_equal(bgr2[b:].cpu().numpy(), np.flip(rgb, 2))
    np.testing.assert_array_equal(dep2[b:].cpu().numpy(), np.flip(dep, 2))
    for buf in (bb, db, mb):             # nothing outside the 2B frames was written
        assert bool((buf[shift + (buf.numel() - shift - 64):] == 0x3C).all()) and bool((buf[:shift] == 0x3C).all())
    if n:
        np.testing.assert_array_equal(m2[:b].cpu().numpy(), masks)
        np.testing.assert_array_equal(m2[b:].cpu().numpy(), np.flip(masks, 3))
        enc = eng.encode(m2).cpu().numpy()
        for i in range(b):
            np.testing.assert_array_equal(enc[b + i].view(np.uint32), u32(encode_np.encode_initial_masks(np.flip(masks[i], 2))))
            np.testing.assert_array_equal(enc[i].view(np.uint32), u32(encode_np.encode_initial_masks(masks[i])))
    eng.close()


# ---- 2. merge kernel, in the four arithmetic modes, eee_mask on and off ----
MASK_KW = dict(eee_mask_on=True, hierarchy=(("eee_mask",), ("eee_boundary",), ("foreground", "center", "offset")))


@pytest.mark.parametrize("eee_mask", [False, True], ids=["boundary", "mask+boundary"])
def test_merge_kernel_bit_exact_all_modes(eee_mask):
    kw = MASK_KW if eee_mask else {}
    h, w, b, n = (64, 96, 1, 3) if eee_mask else (66, 98, 1, 3)          # W % 4 == 0: the 16-byte path; else the scalar one
    batch, offs, image = _scene(3, b, h, w, n)
    sd = arch.init_state_dict(seed=1, loud_heads=True, **kw)
    for mode in (0, 1, 2, 3):
        qc = engine.set_arch(engine.make_config(h, w, max_batch=2 * b, max_instances=n), **kw)
        qc.compute_dtype = mode
        eng = engine.Engine(qc, "cuda:0")
        eng.load_state_dict(sd)
        bgr2, dep2, m2 = two(batch["rgb"]), two(batch["depth"]), two(batch["masks"])
        eng.tta_flip_inputs(bgr2, dep2, m2)
        lg2 = eng.forward(bgr2, dep2, eng.encode(m2))
        merged = eng.tta_merge(lg2)
        assert merged.shape == (b, eng.planes, h, w) and eng.planes == (12 if eee_mask else 8)
        L2 = lg2.cpu().numpy()
        np.testing.assert_array_equal(merged.cpu().numpy().view(np.uint32), tta_merge_np(L2).view(np.uint32))
        assert float(np.abs(L2[:, X_OFFSET_PLANE]).max()) > 0
        eng.close()


# ---- 3. / 5. parity against the oracle ----
_CASE = {}


def _tta_case(h, w, b, n, single=False):
    """Scene, loud weights, and the oracle's heads on x and flip(x) merged by the contract (computed once per configuration)."""
    key = (h, w, b, n, single)
    if key in _CASE:
        return _CASE[key]
    kw = dict(streams=1) if single else {}
    batch, offs, image = _scene(11, b, h, w, n, single)
    sd = loud_state_dict(2, image, offs, n, **kw)
    foffs = np.stack([encode_np.encode_initial_masks(np.flip(m, 2)) for m in batch["masks"]])
    with torch.no_grad():
        ref = _oracle(sd, **kw)(torch.cat([image, image.flip(3)]), torch.from_numpy(np.concatenate([offs, foffs])))
    L2 = torch.cat([ref[k] for k in HEADS], 1).numpy()
    merged = torch.from_numpy(tta_merge_np(L2))
    o = 0
    ref_m = {}
    for k in HEADS:
        c = ref[k].shape[1]
        ref_m[k] = merged[:, o:o + c]
        o += c
    _CASE[key] = (batch, sd, ref_m, kw)
    return _CASE[key]


def _hip_tta(h, w, b, n, mode, batch, sd, kw, single=False):
    qc = engine.set_arch(engine.make_config(h, w, max_batch=2 * b, max_instances=n), **kw)
    qc.compute_dtype = mode
    eng = engine.Engine(qc, "cuda:0")
    eng.load_state_dict(sd)
    from quber_amd.maskrefiner.predictor import RefinerModel
    model = RefinerModel(None, sd, "cuda:0", tta=True)
    bgr2 = two(batch["rgb"])
    dep2 = None if single else two(batch["depth"])
    merged = model.tta_logits(eng, bgr2, dep2, two(batch["masks"]))
    post = eng.postprocess(merged)
    k = int(post["count"].max())
    pm = eng.extract_masks(post, max(k, 1)).cpu().numpy()
    out = merged.cpu(), {key: v.cpu() for key, v in post.items()}, pm
    eng.close()
    return out


def _check_post(merged, post, pm):
    ks = []
    for i in range(merged.shape[0]):
        o = postproc_ref.postprocess(merged[i, 0:1], merged[i, 1:2], merged[i, 2:4])
        k = len(o["labels"])
        ks.append(k)
        np.testing.assert_array_equal(post["panoptic"][i].numpy(), o["panoptic"].numpy())
        assert int(post["count"][i]) == k
        np.testing.assert_array_equal(post["labels"][i, :k].numpy(), o["labels"].numpy())
        if k:
            np.testing.assert_array_equal(post["boxes"][i, :k].numpy(), o["boxes"].numpy())
            np.testing.assert_array_equal(pm[i, :k].astype(bool), o["masks"].numpy())
            np.testing.assert_allclose(post["scores"][i, :k].numpy(), o["scores"].numpy(), rtol=2e-5, atol=1e-6)
    return ks


@pytest.mark.parametrize("h,w,b,n", [(480, 640, 1, 8), (192, 256, 3, 6)], ids=["640x480-b1", "256x192-b3"])
@pytest.mark.parametrize("mode", [0, 3], ids=["f32", "bf16x3"])
def test_tta_parity_against_oracle(h, w, b, n, mode):
    batch, sd, ref_m, kw = _tta_case(h, w, b, n)
    merged, post, pm = _hip_tta(h, w, b, n, mode, batch, sd, kw)
    _check_heads(merged, ref_m, HEADS)
    ks = _check_post(merged, post, pm)
    assert sum(ks) >= b, ks                                  # real instances


def test_tta_single_stream_rgb_only():
    h, w, b, n = 192, 256, 1, 6
    batch, sd, ref_m, kw = _tta_case(h, w, b, n, single=True)
    merged, post, pm = _hip_tta(h, w, b, n, 0, batch, sd, kw, single=True)
    _check_heads(merged, ref_m, HEADS)
    ks = _check_post(merged, post, pm)
    assert sum(ks) >= 1, ks


# ---- 4. flip equivariance ----
@pytest.mark.parametrize("h,w,n", [(192, 256, 6), (480, 640, 8)], ids=["256x192", "640x480"])
@pytest.mark.parametrize("mode", [0, 3], ids=["f32", "bf16x3"])
def test_flip_equivariance(h, w, n, mode):
    """TTA(flip(x)) against flip(TTA(x)) with the x-offset plane negated: both runs feed the network the same two frames, in
    swapped slots, so the two sums hold the same terms - up to how the network's result depends on the slot a frame runs in.
    Bar 1e-5 x max(1, max |logit|); the measured distance is printed (bit-exact at 256x192, a few 1e-5 at 640x480).  No oracle:
    loud heads with a fixed centre bias are enough for a property of the HIP path alone."""
    batch = _scene(11, 1, h, w, n)[0]
    sd = arch.init_state_dict(seed=2, loud_heads=True, center_bias=-1.68)
    qc = engine.make_config(h, w, max_batch=2, max_instances=n)
    qc.compute_dtype = mode
    eng = engine.Engine(qc, "cuda:0")
    eng.load_state_dict(sd)
    from quber_amd.maskrefiner.predictor import RefinerModel
    model = RefinerModel(None, sd, "cuda:0", tta=True)
    flip = {k: np.ascontiguousarray(np.flip(batch[k], 2 if k != "masks" else 3)) for k in ("rgb", "depth", "masks")}
    a = model.tta_logits(eng, two(batch["rgb"]), two(batch["depth"]), two(batch["masks"])).cpu().numpy()
    f = model.tta_logits(eng, two(flip["rgb"]), two(flip["depth"]), two(flip["masks"])).cpu().numpy()
    eng.close()
    fa = mirror_logits_np(f)
    d = float(np.abs(fa - a).max())
    print(f"flip equivariance mode {mode}: max |TTA(flip x) mirrored - TTA(x)| = {d:.3e}, bit-exact = {np.array_equal(u32(fa), u32(a))}")
    assert d <= 1e-5 * max(1.0, float(np.abs(a).max())), d


# ---- 6. hipGraph ----
def test_tta_step_graph_replay_equals_eager():
    """flip -> encode -> forward of 2 frames -> merge -> post-processing captured at B = 1 and replayed == the eager step bit for bit
    (tests/tta_graph_child.py).  The capture and replay run in a fresh child process: the same replay inside the suite's long-lived
    process, after the graph tests of tests/test_gpu_network.py, ended in a host-side segmentation fault inside the runtime's graph
    launch (no GPU fault), while the step captured and replayed correctly in every fresh process."""
    import json
    import os
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tta_graph_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["flip_in_graph"] and res["step_is_tta_logits"] and res["replay_equals_eager"], res
    assert res["instances"] >= 1, res


# ---- 7. public API ----
def test_predictor_and_adapter_with_tta(tmp_path):
    from PIL import Image
    from quber_amd.eval.refiner_model import MaskRefinerTTA
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
    h, w, n = 480, 640, 8
    batch, sd, _, kw = _tta_case(h, w, 1, n)
    pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, tta=True)
    scenes = [synth.make_scene(60 + i, h, w, n) for i in range(2)]
    rgb = np.stack([batch["rgb"][0]] + [s["rgb"] for s in scenes])
    dep = np.stack([batch["depth"][0]] + [s["depth"] for s in scenes])
    masks = [batch["masks"][0]] + [s["masks"] for s in scenes]
    out = pred.predict(rgb[0], dep[0], masks[0])[0]
    # the engine-level step on the same frame
    model = pred.model
    eng = model.engine_for(h, w, 2, n)
    merged = model.tta_logits(eng, two(rgb[:1]), two(dep[:1]), two(masks[0][None]))
    post = eng.postprocess(merged)
    k = int(post["count"][0])
    assert k >= 1 and "instances" in out
    assert torch.equal(out["sem_seg"], merged[0, 0:1]) and torch.equal(out["eee_boundary"], merged[0, 4:8])
    assert torch.equal(out["panoptic_seg"][0], post["panoptic"][0])
    inst = out["instances"]
    assert torch.equal(inst.pred_masks, eng.extract_masks(post, k)[0].bool())
    assert torch.equal(inst.scores, post["scores"][0, :k]) and torch.equal(inst.pred_boxes.tensor, post["boxes"][0, :k])
    # predict_batch of 3 frames against 3 predict calls: the batch-invariance level (profiles/r20_batch_invariance.txt)
    one = [out] + [pred.predict(rgb[i], dep[i], masks[i])[0] for i in (1, 2)]
    many = pred.predict_batch(rgb, dep, masks)
    for o1, ob in zip(one, many):
        assert float((o1["sem_seg"] - ob["sem_seg"]).abs().max()) < 1e-4
        assert float((o1["eee_boundary"] - ob["eee_boundary"]).abs().max()) < 1e-4
        assert float((o1["panoptic_seg"][0] == ob["panoptic_seg"][0]).float().mean()) > 0.9999
    pred.model.close()
    # the reference driver's refiner on files; predict_stream(batch=2) on top
    items = []
    for i in range(3):
        Image.fromarray(rgb[i][:, :, ::-1].copy()).save(tmp_path / f"rgb{i}.png")
        Image.fromarray(dep[i][:, :, 0].astype(np.uint16) * 5 + 300).save(tmp_path / f"depth{i}.png")
        items.append((str(tmp_path / f"rgb{i}.png"), str(tmp_path / f"depth{i}.png"), masks[i] != 0, None))
    ref = MaskRefinerTTA(None, weights_file=None, dataset="OSD")
    assert ref.refiner_predictor.tta
    ref.refiner_predictor.model.state_dict = sd
    ref.refiner_predictor.model._engines.clear()
    seq = [ref.predict(*it) for it in items]
    assert sum(len(r[0]) for r in seq) >= 1 and all(r[2] > 0 for r in seq)
    got = list(ref.predict_stream(items, workers=2, batch=2))                    # 2 + 1 frames, engines of 4 frames
    assert len(got) == 3
    assert ref.refiner_predictor.model.engine_for(h, w, 1).qcfg.max_batch == 4
    for (m0, o0, _, _), (m1, o1, _, _) in zip(seq, got):
        assert float((o0["sem_seg"] - o1["sem_seg"]).abs().max()) < 1e-4
        assert float((o0["panoptic_seg"][0] == o1["panoptic_seg"][0]).float().mean()) > 0.9999
    ref.refiner_predictor.model.close()
