"""GPU: the HIP network (a3-a7) against the pure-torch oracle restatement, fp32, tolerance 1e-4."""
import numpy as np
import pytest
import torch

from oracle.network_torch import ArchCfg, MaskRefinerNet
from oracle import encode_np, postproc_ref
from quber_amd import _lib, arch, engine, synth
from quber_amd.maskrefiner.predictor import MaskRefinerPredictor

pytestmark = pytest.mark.gpu

TOL = 1e-4   # BASELINE.json north_star: float outputs within 1e-4 of the reference CPU path


def oracle_cfg(**kw):
    kw = dict(kw)
    if "hierarchy" in kw:
        kw["hierarchy"] = [list(l) for l in kw["hierarchy"]]
    if "fusion_target" in kw:
        kw["fusion_target"] = list(kw["fusion_target"])
    return ArchCfg(**kw)


def oracle_net(sd, depth=50, **kw):
    net = MaskRefinerNet(oracle_cfg(depth=depth, **kw)).eval()
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    return net


def inputs(seed, b, h, w, n):
    batch = synth.make_batch(seed, b, h, w, n)
    offs = np.stack([encode_np.encode_initial_masks(m) for m in batch["masks"]])
    return batch, offs


def loud_state_dict_hip(seed, sc, h, w, n):
    """Loud predictors (arch.init_state_dict(loud_heads=True): O(1) logits that depend on the features) with the centre bias
    calibrated on the HIP path's own centre logits of scene `sc`, so that ~n maxima pass the 0.3 threshold and a8-a11 see real
    instances.  (The reference's N(0, 0.001) predictor init gives |logits| ~ 3e-3 and K = 0: "< 1e-4" is then a 3 % relative check on
    an empty scene.)"""
    e0 = engine.Engine(engine.make_config(h, w, max_batch=1, max_instances=max(n, 1)), "cuda:0")
    e0.load_state_dict(arch.init_state_dict(seed=seed, loud_heads=True))
    offs = e0.encode(torch.from_numpy((sc["masks"] != 0).astype(np.uint8)[None]).cuda())
    lg0 = e0.forward(torch.from_numpy(sc["rgb"][None]).cuda(), torch.from_numpy(sc["depth"][None]).cuda(), offs)
    bias = arch.calibrate_center_bias(lg0[:, 1:2].float().cpu(), n)
    e0.close()
    return arch.init_state_dict(seed=seed, loud_heads=True, center_bias=bias)


def rel_err(got, ref):
    return float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))


@pytest.mark.parametrize("h,w,b,depth", [(64, 96, 2, 50), (128, 160, 1, 50), (64, 64, 1, 101), (70, 102, 2, 50), (53, 75, 1, 50)])
def test_network_vs_oracle_small(h, w, b, depth):
    # loud predictors (O(1) logits that depend on the features): with the reference's N(0, 0.001) init the logits are ~3e-3 and an
    # absolute 1e-4 bar on them checks little (the taps below are relative either way)
    sd = arch.init_state_dict(seed=1, depth=depth, loud_heads=True)
    net = oracle_net(sd, depth)
    batch, offs = inputs(3, b, h, w, 4)
    qc = engine.make_config(h, w, max_batch=b + 1)
    qc.resnet_depth = depth
    eng = engine.Engine(qc, "cuda:0")
    eng.load_state_dict(sd)
    bgr, dep = torch.from_numpy(batch["rgb"]).cuda(), torch.from_numpy(batch["depth"]).cuda()
    logits = eng.forward(bgr, dep, torch.from_numpy(offs).cuda()).cpu()
    image = torch.cat([torch.from_numpy(batch["rgb"]), torch.from_numpy(batch["depth"])], -1).permute(0, 3, 1, 2)
    taps = {}
    with torch.no_grad():
        ref = net(image, torch.from_numpy(offs), taps)
    for name in ("res2", "res3", "res5", "y", "feat_eee_boundary", "z1", "feat_center"):
        got = eng.debug_tensor(name, b).cpu().permute(0, 3, 1, 2)
        assert rel_err(got, taps[name]) < TOL, name
    exp = torch.cat([ref["foreground"], ref["center"], ref["offset"], ref["eee_boundary"]], 1)
    assert logits.shape == exp.shape and float(exp[:, 0].abs().max()) > 0.5
    d = (logits - exp).abs()
    assert float(d[:, :2].max()) < TOL and float(d[:, 2:4].max()) < 4 * TOL and float(d[:, 4:].max()) < TOL      # head units: offsets are emitted x4 (model.py:700)
    if depth == 50 and h % 16 == 0 and w % 16 == 0:
        assert abs(eng.forward_flops() / 2e9 - 187.8 * (h * w) / (480 * 640)) < 0.02 * 187.8 * (h * w) / (480 * 640)
    eng.close()


VARIANTS = {
    # run_eval.py's default config: ...-hf-m-b-f-c-o-l3-e2-b8.yaml (5 levels, 2 error classes, mask + boundary)
    "m-b-f-c-o-e2": dict(eee_mask_on=True, error_classes=2, fusion_target=("pred", "feat"),
                         hierarchy=(("eee_mask",), ("eee_boundary",), ("foreground",), ("center",), ("offset",))),
    "m-b-fco-feat": dict(eee_mask_on=True, fusion_target=("feat",),
                         hierarchy=(("eee_mask",), ("eee_boundary",), ("foreground", "center", "offset"))),
    "bfco-single-level": dict(hierarchy=(("eee_boundary", "foreground", "center", "offset"),)),
    "noeee-flat": dict(hierarchical=False, eee_boundary_on=False, error_classes=2),
    "mb-fco-e33-pred": dict(eee_mask_on=True, error_classes=3, fusion_target=("pred",),
                            hierarchy=(("eee_mask", "eee_boundary"), ("foreground", "center", "offset"))),
    "l0-backbone-fusion": dict(backbone_fusion_layers=0),
    "single-stream": dict(streams=1),
    "add-fusion-l3": dict(fusion_add=True, backbone_fusion_layers=3),    # Base-Mask-Refiner.yaml's own defaults
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_head_hierarchy_variants(name):
    kw = VARIANTS[name]
    h, w, b = 64, 96, 2
    sd = arch.init_state_dict(seed=4, **kw)
    net = oracle_net(sd, **kw)
    batch, offs = inputs(5, b, h, w, 3)
    qc = engine.set_arch(engine.make_config(h, w, max_batch=b), **kw)
    eng = engine.Engine(qc, "cuda:0")
    assert sorted(n for n, _ in eng.weight_specs()) == sorted(sd)
    eng.load_state_dict(sd)
    single = kw.get("streams", 2) == 1
    logits = eng.forward(torch.from_numpy(batch["rgb"]).cuda(), None if single else torch.from_numpy(batch["depth"]).cuda(),
                         torch.from_numpy(offs).cuda()).cpu()
    image = torch.cat([torch.from_numpy(batch["rgb"])] + ([] if single else [torch.from_numpy(batch["depth"])]), -1).permute(0, 3, 1, 2)
    with torch.no_grad():
        ref = net(image, torch.from_numpy(offs))
    parts = [ref["foreground"], ref["center"], ref["offset"]]
    parts += [ref["eee_boundary"]] if "eee_boundary" in ref else []
    parts += [ref["eee_mask"]] if "eee_mask" in ref else []
    exp = torch.cat(parts, 1)
    assert logits.shape == exp.shape
    assert float((logits - exp).abs().max()) < TOL
    eng.close()


def test_reference_default_yaml_loads(tmp_path):
    # the yaml text below restates the keys of the reference's run_eval.py default config over its base file
    (tmp_path / "Base.yaml").write_text(
        "MODEL:\n  META_ARCHITECTURE: MaskRefiner\n  BACKBONE:\n    NAME: build_resnet_deeplab_rgbd_fusion_backbone\n"
        "    FUSION_STRATEGY: add\n    NUM_FUSION_LAYERS: 3\n  RESNETS:\n    OUT_FEATURES: [res2, res3, res5]\n    RES5_DILATION: 2\n"
        "  PIXEL_MEAN: [103.53, 116.28, 123.675, 127.5, 127.5, 127.5]\n  PIXEL_STD: [1, 1, 1, 1, 1, 1]\n"
        "  INS_EMBED_HEAD:\n    NAME: MaskRefinerInsEmbedHead\n    NORM: GN\n    EEE_MASK_ON: True\n    EEE_BOUNDARY_ON: True\n    ERROR_TYPE: e2\n"
        "  PANOPTIC_DEEPLAB:\n    CENTER_THRESHOLD: 0.3\n    STUFF_AREA: 2048\nINPUT:\n  OFFSET_INPUT_ON: True\n  DEPTH_ON: True\n")
    (tmp_path / "default.yaml").write_text(
        "_BASE_: Base.yaml\nMODEL:\n  BACKBONE:\n    FUSION_STRATEGY: concat\n    NUM_FUSION_LAYERS: 2\n  INS_EMBED_HEAD:\n"
        "    HIERARCHICAL_FUSION_ON: True\n    HIERARCHY: [[eee_mask], [eee_boundary], [foreground], [center], [offset]]\n"
        "    NUM_FUSION_LAYERS: 3\n    FUSION_TARGET: [pred, feat]\n    ERROR_TYPE: e2\n")
    pred = MaskRefinerPredictor(str(tmp_path / "default.yaml"), seed=1)
    sc = synth.make_scene(2, 64, 96, 2)
    r = pred.predict(sc["rgb"], sc["depth"], sc["masks"])[0]
    assert r["eee_mask"].shape == (2, 64, 96) and r["eee_boundary"].shape == (2, 64, 96)


def test_network_vs_oracle_full_frame_and_predictor():
    h, w, n = 480, 640, 8          # BASELINE.json configs[0]: one 640x480 frame + 8 initial masks through maskrefiner.predictor
    sc = synth.make_scene(5, h, w, n)
    sd = loud_state_dict_hip(2, sc, h, w, n)
    pred = MaskRefinerPredictor(None, state_dict=sd)
    net = oracle_net(sd)
    out = pred.predict(sc["rgb"], sc["depth"], sc["masks"])
    assert isinstance(out, list) and len(out) == 1
    r = out[0]
    assert r["sem_seg"].shape == (1, h, w) and r["eee_boundary"].shape == (4, h, w)
    assert r["panoptic_seg"][0].shape == (h, w) and r["panoptic_seg"][1] is None
    offs = encode_np.encode_initial_masks(sc["masks"])[None]
    image = torch.from_numpy(np.concatenate([sc["rgb"], sc["depth"]], -1)).permute(2, 0, 1)[None]
    with torch.no_grad():
        ref = net(image, torch.from_numpy(offs))
    assert float((r["sem_seg"].cpu() - ref["foreground"][0]).abs().max()) < TOL
    assert float((r["eee_boundary"].cpu() - ref["eee_boundary"][0]).abs().max()) < TOL
    # the detectron2-style entry point gives the same result as predict()
    r2 = pred.model([{"image": image[0], "height": h, "width": w, "initial_pred_offset": torch.from_numpy(offs[0])}])[0]
    assert torch.equal(r2["sem_seg"], r["sem_seg"]) and torch.equal(r2["panoptic_seg"][0], r["panoptic_seg"][0])
    # post-processing of the HIP logits through the oracle gives the HIP label map bit for bit
    eng = pred.model.engine_for(h, w, 1)
    lg = eng.forward(torch.from_numpy(sc["rgb"][None]).cuda(), torch.from_numpy(sc["depth"][None]).cuda(),
                     torch.from_numpy(offs).cuda()).cpu()
    assert float(lg[0, 0].abs().max()) > 0.5                      # the heads are loud
    o = postproc_ref.postprocess(lg[0, 0:1], lg[0, 1:2], lg[0, 2:4])
    np.testing.assert_array_equal(r["panoptic_seg"][0].cpu().numpy(), o["panoptic"].numpy())
    assert len(o["labels"]) >= 1 and "instances" in r             # real instances reach a8-a11 through predict()
    inst = r["instances"].to("cpu")
    np.testing.assert_array_equal(inst.pred_masks.numpy(), o["masks"].numpy())
    assert inst.pred_masks.dtype == torch.bool and list(inst.pred_classes) == list(o["classes"])


def test_adapter_from_files(tmp_path):
    """eval/refiner_model.py:MaskRefiner drop-in: paths in, (masks, output, seconds, fg_mask) out."""
    from PIL import Image
    from quber_amd.eval.refiner_model import MaskRefiner
    sc = synth.make_scene(9, 480, 640, 6)
    Image.fromarray(sc["rgb"][:, :, ::-1].copy()).save(tmp_path / "rgb.png")
    depth_mm = (sc["depth"][:, :, 0].astype(np.uint16) * 5 + 300)
    depth_mm[:10, :10] = 0
    Image.fromarray(depth_mm).save(tmp_path / "depth.png")
    np.save(tmp_path / "depth.npy", depth_mm.astype(np.float32) / 1000.0)
    ref = MaskRefiner(None, None, dataset="OCID")
    for dpath in ("depth.png", "depth.npy"):
        masks, out, secs, fg = ref.predict(str(tmp_path / "rgb.png"), str(tmp_path / dpath), sc["masks"] != 0, None)
        assert fg is None and secs > 0 and "sem_seg" in out and "panoptic_seg" in out
        if len(masks):
            assert masks.dtype == np.bool_ and masks.shape[1:] == (480, 640)
            assert not masks[:, :10, :10].any()            # OCID zero-depth masking (refiner_model.py:279-288)


def test_adapter_stream_equals_sequential(tmp_path):
    """MaskRefiner.predict_stream: the host side of frame i + 1 (file decoding, resize, TELEA in-painting) on a worker
    thread while frame i is refined - the same results as predict() called frame after frame, in the same order."""
    from PIL import Image
    from quber_amd.eval.refiner_model import MaskRefiner
    items = []
    for i in range(4):
        sc = synth.make_scene(20 + i, 480, 640, 5)
        Image.fromarray(sc["rgb"][:, :, ::-1].copy()).save(tmp_path / f"rgb{i}.png")
        depth_mm = (sc["depth"][:, :, 0].astype(np.uint16) * 5 + 300)
        depth_mm[40 + 10 * i:70 + 10 * i, 100:180] = 0                      # a hole to in-paint
        Image.fromarray(depth_mm).save(tmp_path / f"depth{i}.png")
        items.append((str(tmp_path / f"rgb{i}.png"), str(tmp_path / f"depth{i}.png"), sc["masks"] != 0, None))
    ref = MaskRefiner(None, None, dataset="OSD")
    seq = [ref.predict(*it) for it in items]
    got = list(ref.predict_stream(items))
    assert len(got) == len(seq)
    for (m0, o0, _, _), (m1, o1, _, _) in zip(seq, got):
        np.testing.assert_array_equal(np.asarray(m0), np.asarray(m1))
        assert torch.equal(o0["sem_seg"], o1["sem_seg"]) and torch.equal(o0["panoptic_seg"][0], o1["panoptic_seg"][0])


def test_adapter_stream_batched(tmp_path):
    """MaskRefiner.predict_stream(items, workers, batch=k): k frames per engine call, one batch in flight while the previous one is
    copied out - the tuples of predict() called frame after frame, in order.  With loud heads (real instances).  A frame's logits
    in a batch-k launch may differ from its batch-1 logits in the last bits (the split-K partition follows the launch size; same
    plan, same arithmetic class): the label maps must agree on >= 99.999 % of the pixels and every differing pixel must be a
    float64 near-tie of the decision that produced it (oracle/fp64_anchor.py: explain_label_flips)."""
    from PIL import Image
    from oracle import fp64_anchor as fa
    from quber_amd.eval.refiner_model import MaskRefiner
    n_frames, n = 10, 6
    items = []
    for i in range(n_frames):
        sc = synth.make_scene(40 + i, 480, 640, n)
        Image.fromarray(sc["rgb"][:, :, ::-1].copy()).save(tmp_path / f"rgb{i}.png")
        depth_mm = (sc["depth"][:, :, 0].astype(np.uint16) * 5 + 300)
        depth_mm[40 + 10 * i:70 + 10 * i, 100:180] = 0                      # a hole to in-paint
        Image.fromarray(depth_mm).save(tmp_path / f"depth{i}.png")
        items.append((str(tmp_path / f"rgb{i}.png"), str(tmp_path / f"depth{i}.png"), sc["masks"] != 0, None))
    sd = arch.init_state_dict(seed=0, loud_heads=True, center_bias=-1.68)
    ref = MaskRefiner(None, None, dataset="OSD")
    model = ref.refiner_predictor.model
    model.state_dict = sd
    model._engines.clear()
    seq = [ref.predict(*it) for it in items]
    got = list(ref.predict_stream(items, workers=4, batch=4))              # 4 + 4 + 2 frames
    assert len(got) == n_frames and sum(len(r[0]) for r in seq) >= n_frames       # real instances
    differing = []
    px = 0
    for i, ((m0, o0, s0, _), (m1, o1, s1, _)) in enumerate(zip(seq, got)):
        assert s0 > 0 and s1 > 0
        assert float((o0["sem_seg"] - o1["sem_seg"]).abs().max()) < TOL and float((o0["eee_boundary"] - o1["eee_boundary"]).abs().max()) < TOL
        p0, p1 = o0["panoptic_seg"][0], o1["panoptic_seg"][0]
        nd = int((p0 != p1).sum())
        px += nd
        if nd:
            differing.append(i)
        else:
            np.testing.assert_array_equal(np.asarray(m0), np.asarray(m1))
            assert torch.equal(o0["instances"].pred_boxes.tensor, o1["instances"].pred_boxes.tensor) if "instances" in o0 else "instances" not in o1
    assert px <= 1e-5 * n_frames * 480 * 640, f"{px} pixels differ"
    # every differing pixel: a float64 near-tie.  The logits of both launch sizes, from the engine the adapter used.
    if differing:
        frs = [ref._load(*items[i][:3]) for i in differing]
        eng = model.engine_for(480, 640, 4, n)
        image = torch.from_numpy(np.stack([np.concatenate([f["rgb"], f["depth"]], -1) for f in frs])).permute(0, 3, 1, 2)
        offs = np.stack([encode_np.encode_initial_masks((f["masks"] != 0).astype(np.uint8)) for f in frs])
        o64 = {j: fa.cat_heads(o)[0] for j, o, _ in fa.oracle64(sd, image, offs, want_taps=())}
        for j, (i, f) in enumerate(zip(differing, frs)):
            a0 = (i // 4) * 4                                               # the batch the stream put the frame in
            grp = [ref._load(*items[q][:3]) for q in range(a0, min(a0 + 4, n_frames))]
            d = lambda key: torch.from_numpy(np.stack([np.ascontiguousarray(g[key]) for g in grp])).cuda()
            mk = torch.from_numpy(np.stack([(g["masks"] != 0).astype(np.uint8) for g in grp])).cuda()
            lg_b = eng.forward(d("rgb"), d("depth"), eng.encode(mk))[i - a0].cpu()
            lg_1 = eng.forward(d("rgb")[i - a0:i - a0 + 1], d("depth")[i - a0:i - a0 + 1], eng.encode(mk[i - a0:i - a0 + 1]))[0].cpu()
            rep = fa.explain_label_flips(lg_b, lg_1, o64[j], pan_hip=got[i][1]["panoptic_seg"][0].cpu())
            print(f"\n[stream batch 4] frame {i}: {rep}")


def test_adapter_armbench_branch(tmp_path):
    """eval/refiner_model.py:226-244: RGB only, image resized to shortest edge 800 / longest 1333 with cv2.resize, the
    initial masks with INTER_NEAREST, refined masks returned at THAT size, fg_mask None."""
    from PIL import Image
    from quber_amd.eval.refiner_model import MaskRefiner, resize_shortest_edge_shape
    from oracle import adapter_np
    sc = synth.make_scene(3, 300, 400, 4)
    Image.fromarray(sc["rgb"][:, :, ::-1].copy()).save(tmp_path / "rgb.png")
    cfg = tmp_path / "rgb_only.yaml"
    cfg.write_text(
        "MODEL:\n  META_ARCHITECTURE: MaskRefiner\n  BACKBONE:\n    NAME: build_resnet_deeplab_fusion_backbone\n"
        "  RESNETS:\n    OUT_FEATURES: [res2, res3, res5]\n    RES5_DILATION: 2\n"
        "  PIXEL_MEAN: [103.53, 116.28, 123.675]\n  PIXEL_STD: [1, 1, 1]\n"
        "  INS_EMBED_HEAD:\n    NAME: MaskRefinerInsEmbedHead\n    NORM: GN\n    HIERARCHICAL_FUSION_ON: True\n"
        "    EEE_BOUNDARY_ON: True\n    HIERARCHY: [[eee_boundary], [foreground, center, offset]]\n"
        "    FUSION_TARGET: [feat, pred]\n    ERROR_TYPE: e3\n"
        "  PANOPTIC_DEEPLAB:\n    CENTER_THRESHOLD: 0.3\n    STUFF_AREA: 2048\nINPUT:\n  OFFSET_INPUT_ON: True\n  DEPTH_ON: False\n  RGB_ON: True\n")
    assert resize_shortest_edge_shape(300, 400) == (800, 1067)
    ref = MaskRefiner(str(cfg), None, dataset="armbench")
    masks, out, secs, fg = ref.predict(str(tmp_path / "rgb.png"), None, sc["masks"] != 0, None)
    assert fg is None and secs > 0
    assert out["sem_seg"].shape == (1, 800, 1067) and out["panoptic_seg"][0].shape == (800, 1067)
    if len(masks):
        assert masks.dtype == np.bool_ and masks.shape[1:] == (800, 1067)
    # the branch's own pre-processing: what the predictor saw is cv2's resize of the inputs
    eng = ref.refiner_predictor.model.engine_for(800, 1067, 1)
    m255 = np.uint8(sc["masks"] != 0) * 255
    exp_masks = np.stack([adapter_np.cv2_resize_nearest(m, 1067, 800) for m in m255])
    got_off = eng.encode(torch.from_numpy(exp_masks[None]).cuda()).cpu().numpy()[0]
    np.testing.assert_array_equal(got_off, encode_np.encode_initial_masks(exp_masks))
    # the batched stream on this branch: RGB only (no depth tensor), frames of TWO sizes -> a group never mixes sizes, order kept
    from PIL import Image as _I
    sc2 = synth.make_scene(4, 240, 400, 3)
    _I.fromarray(sc2["rgb"][:, :, ::-1].copy()).save(tmp_path / "rgb2.png")
    a_item = (str(tmp_path / "rgb.png"), None, sc["masks"] != 0, None)
    b_item = (str(tmp_path / "rgb2.png"), None, sc2["masks"] != 0, None)
    seq = [ref.predict(*it) for it in (a_item, a_item, b_item, a_item)]
    got = list(ref.predict_stream([a_item, a_item, b_item, a_item], workers=2, batch=2))
    assert [g[1]["sem_seg"].shape for g in got] == [q[1]["sem_seg"].shape for q in seq]
    for (m0, o0, _, f0), (m1, o1, _, f1) in zip(seq, got):
        assert f0 is None and f1 is None
        assert float((o0["sem_seg"] - o1["sem_seg"]).abs().max()) < TOL
        assert (o0["panoptic_seg"][0] != o1["panoptic_seg"][0]).float().mean() < 1e-5


@pytest.mark.parametrize("dtype", [0, 3, 2], ids=["f32", "bf16x3", "f16"])
def test_side_lanes_equal_one_stream(dtype):
    """Batches <= 16 (exact fp32 and bf16x3: <= 12) run the fusion convolutions of res2 / res3 on side streams of the context beside the later ResNet stages
    (csrc/plan.hip: Builder::fork / join).  The results must equal the one-stream forward bit for bit - same launches, same
    split-K choices, own workspaces per lane - and stay equal over repeated runs (no race on a shared buffer), also on an
    engine built for a larger batch."""
    lib = _lib.load()
    h, w, n = 480, 640, 12
    sd = arch.init_state_dict(seed=3, loud_heads=True, center_bias=-1.6)
    qc = engine.make_config(h, w, max_batch=16, max_instances=n)
    qc.compute_dtype = dtype
    eng = engine.Engine(qc, "cuda:0")
    eng.load_state_dict(sd)
    try:
        for b in (1, 2, 5, 12, 16):
            batch = synth.make_batch(50 + b, b, h, w, n)
            bgr, dep = torch.from_numpy(batch["rgb"]).cuda(), torch.from_numpy(batch["depth"]).cuda()
            off = eng.encode(torch.from_numpy(batch["masks"]).cuda())
            eng.set_option(24, 0)
            one = eng.forward(bgr, dep, off).clone()
            taps = {k: eng.debug_tensor(k, b).clone() for k in ("res2", "res3", "res5", "y")}
            eng.set_option(24, 1)
            for _ in range(12):
                assert torch.equal(eng.forward(bgr, dep, off), one)
            for k, v in taps.items():
                assert torch.equal(eng.debug_tensor(k, b), v), k
    finally:
        eng.close()


@pytest.mark.parametrize("dtype,b,off_key,rel", [(2, 12, 32, 2.5 * 2.0 ** -10), (2, 15, 32, 2.5 * 2.0 ** -10), (3, 15, 35, 2e-6)],
                         ids=["f16-12", "f16-15", "bf16x3-15"])
def test_run_of_tiles_across_the_stream_boundary(dtype, b, off_key, rel):
    """Regression (round 6, profiles/r20_h8_affine_race.md).  The persistent LDS-DMA kernels (csrc/conv_h8.hip: fp16 data path; csrc/conv_x8.hip:
    bf16x3 mode) hand every block a run of tiles; a launch of the two-stream backbone holds the RGB stream's tiles, then the depth stream's, and
    when tiles % 8 != 0 the run of some blocks crosses from one stream to the other (640x480: batches 9, 11, 12, 14, 15 - never 8 or 16, which
    every other test and the bench use).  Wave 0 then requested the next-but-one tile's scale / shift vectors into the LDS image that late
    waves were still reading in the epilogue of the tile before: the bottleneck projections of res3 (conv3 + shortcut as one GEMM: 900 tiles at
    batch 12; conv1, 128 channels: 564 at batch 15) came out differently from run to run, 0.03-0.8 off at the res3 tap.  Now: three images in turn.
    Bars: repeated forwards are bit-equal, and the taps agree with the same network with those kernels switched off (fp16: key 32, no launch has
    that many tiles - within two fp16 steps; bf16x3: key 35 = 0 - the same partial products in the same order on conv_igemm.hip)."""
    h, w, n = 480, 640, 12
    sd = arch.init_state_dict(seed=3, loud_heads=True, center_bias=-1.6)
    batch = synth.make_batch(70 + b, b, h, w, n)
    outs = []
    for off in (False, True):
        qc = engine.make_config(h, w, max_batch=b, max_instances=n)
        qc.compute_dtype = dtype
        eng = engine.Engine(qc, "cuda:0")
        if off:
            eng.set_option(off_key, (1 << 20) if off_key == 32 else 0)
        eng.set_option(24, 0)                      # one stream: the launches in plan order
        eng.load_state_dict(sd)
        try:
            bgr, dep = torch.from_numpy(batch["rgb"]).cuda(), torch.from_numpy(batch["depth"]).cuda()
            off_t = eng.encode(torch.from_numpy(batch["masks"]).cuda())
            first = eng.forward(bgr, dep, off_t).clone()
            taps = {k: eng.debug_tensor(k, b).clone().float() for k in ("res2", "res3", "res5", "y")}
            for _ in range(5):
                assert torch.equal(eng.forward(bgr, dep, off_t), first)
                for k, v in taps.items():
                    assert torch.equal(eng.debug_tensor(k, b).float(), v), k
            outs.append(taps)
        finally:
            eng.close()
    for k, v in outs[0].items():
        assert float((v - outs[1][k]).abs().max()) <= rel * float(v.abs().max()), k


@pytest.mark.parametrize("dtype", [0, 3], ids=["f32", "bf16x3"])
def test_frames_of_an_odd_batch_equal_the_frames_one_by_one(dtype):
    """No operation of the path crosses frames (GroupNorm is per image), so a frame's logits in a batch of 11 - a batch size
    whose launches have tile counts that are no multiple of the 8 XCDs, ragged last tiles and runs of tiles that cross from the RGB to the depth
    stream (profiles/r20_h8_affine_race.md: a launch structure only such batches produce) - may differ from the same frame refined alone by the
    re-association of fp32 sums only (tile and split-K choices follow the batch).  Bar: 1e-5 of the logit scale on every frame
    (measured 3-4e-6 at every batch 3-16: profiles/r20_batch_invariance.txt); a tile scaled, skipped or computed twice is orders above."""
    h, w, n, b = 480, 640, 12, 11
    sd = arch.init_state_dict(seed=3, loud_heads=True, center_bias=-1.6)
    batch = synth.make_batch(90, b, h, w, n)
    bgr, dep, masks = (torch.from_numpy(batch[k]).cuda() for k in ("rgb", "depth", "masks"))
    outs = []
    for maxb in (1, b):
        qc = engine.make_config(h, w, max_batch=maxb, max_instances=n)
        qc.compute_dtype = dtype
        eng = engine.Engine(qc, "cuda:0")
        eng.load_state_dict(sd)
        try:
            if maxb == 1:
                outs.append(torch.cat([eng.forward(bgr[i:i + 1], dep[i:i + 1], eng.encode(masks[i:i + 1])).clone() for i in range(b)]))
            else:
                outs.append(eng.forward(bgr, dep, eng.encode(masks)).clone())
        finally:
            eng.close()
    scale = float(outs[0].abs().max())
    assert scale > 5.0                                # loud heads: the bar means something
    per_frame = (outs[1] - outs[0]).abs().amax((1, 2, 3))
    assert float(per_frame.max()) <= 1e-5 * scale, per_frame.tolist()


def test_config2_1280x720_hipgraph_steady_state():
    """BASELINE.json configs[2]: 1280x720, 30 instances, the whole step captured in one hipGraph.  The replayed graph must
    give the eager results bit for bit on new inputs (it reads the device buffers, not captured values), the logits match
    the oracle within 1e-4 and the label map is the oracle's post-processing of those logits."""
    h, w, n = 720, 1280, 30
    sd = loud_state_dict_hip(4, synth.make_scene(12, h, w, n), h, w, n)     # loud heads, centre bias calibrated on the frame the replay refines
    eng = engine.Engine(engine.make_config(h, w, max_batch=1, max_instances=n), "cuda:0")
    eng.load_state_dict(sd)
    dev = "cuda:0"
    masks = torch.empty((1, n, h, w), dtype=torch.uint8, device=dev)
    bgr = torch.empty((1, h, w, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((1, h, w, 3), dtype=torch.uint8, device=dev)
    offsets = torch.empty((1, 3, h, w), dtype=torch.float32, device=dev)
    logits = torch.empty((1, eng.planes, h, w), dtype=torch.float32, device=dev)
    post = eng.alloc_post(1)
    max_inst = min(eng.cap, n + 12)
    out_masks = torch.empty((1, max_inst, h, w), dtype=torch.uint8, device=dev)

    def load(seed):
        sc = synth.make_scene(seed, h, w, n)
        masks.copy_(torch.from_numpy(sc["masks"][None]))
        bgr.copy_(torch.from_numpy(sc["rgb"][None]))
        depth.copy_(torch.from_numpy(sc["depth"][None]))
        return sc

    def step():
        eng.encode(masks, offsets)
        eng.forward(bgr, depth, offsets, logits)
        eng.postprocess(logits, post)
        eng.extract_masks(post, max_inst, out_masks)

    load(11)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    sc = load(12)                      # new frame: the graph was captured on frame 11
    step()
    torch.cuda.synchronize()
    eager = (logits.clone(), post["panoptic"].clone(), post["count"].clone(), out_masks.clone())
    for t in (logits, post["panoptic"], out_masks):
        t.zero_()
    graph.replay()
    graph.replay()                     # steady state: replays are idempotent
    torch.cuda.synchronize()
    assert torch.equal(logits, eager[0]) and torch.equal(post["panoptic"], eager[1])
    assert torch.equal(post["count"], eager[2]) and torch.equal(out_masks, eager[3])
    # against the oracle
    net = oracle_net(sd)
    offs = encode_np.encode_initial_masks(sc["masks"])[None]
    np.testing.assert_array_equal(offsets.cpu().numpy(), offs)
    image = torch.from_numpy(np.concatenate([sc["rgb"], sc["depth"]], -1)).permute(2, 0, 1)[None]
    with torch.no_grad():
        ref = net(image, torch.from_numpy(offs))
    exp = torch.cat([ref["foreground"], ref["center"], ref["offset"], ref["eee_boundary"]], 1)
    lg = logits.cpu()
    d = (lg - exp).abs()
    assert float(lg[0, 0].abs().max()) > 0.5                      # the heads are loud
    # head units: the offset planes are emitted x4 (model.py:700)
    assert float(d[:, :2].max()) < TOL and float(d[:, 2:4].max()) < 4 * TOL and float(d[:, 4:].max()) < TOL
    o = postproc_ref.postprocess(lg[0, 0:1], lg[0, 1:2], lg[0, 2:4])
    np.testing.assert_array_equal(post["panoptic"][0].cpu().numpy(), o["panoptic"].numpy())
    k = int(post["count"][0])
    assert k >= 1 and k == len(o["labels"])                       # the graph replay delivered real instances ...
    np.testing.assert_array_equal(out_masks[0, :k].cpu().numpy().astype(bool), o["masks"].numpy())     # ... and their masks


@pytest.mark.parametrize("dtype,b", [(0, 6), (3, 6), (2, 16)], ids=["f32-6", "bf16x3-6", "f16-16"])
def test_hipgraph_replay_with_side_lanes_at_larger_batches(dtype, b):
    """Since round 6's last pass the side lanes run up to 16 frames (fp32-class modes: 12): a step captured at such a batch holds the lanes'
    fork / join events inside the hipGraph (bench.py captures the step at N > 1; predict_stream users may).  The replay on NEW inputs must
    equal the eager step bit for bit, twice over (csrc/api.hip quber_forward: event record / wait on the context's own streams are capturable)."""
    h, w, n = 240, 320, 6
    sd = arch.init_state_dict(seed=3, loud_heads=True, center_bias=-1.6)
    qc = engine.make_config(h, w, max_batch=b, max_instances=n)
    qc.compute_dtype = dtype
    eng = engine.Engine(qc, "cuda:0")
    eng.load_state_dict(sd)
    dev = "cuda:0"
    masks = torch.empty((b, n, h, w), dtype=torch.uint8, device=dev)
    bgr = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev)
    offsets = torch.empty((b, 3, h, w), dtype=torch.float32, device=dev)
    logits = torch.empty((b, eng.planes, h, w), dtype=torch.float32, device=dev)
    post = eng.alloc_post(b)

    def load(seed):
        batch = synth.make_batch(seed, b, h, w, n)
        masks.copy_(torch.from_numpy(batch["masks"]))
        bgr.copy_(torch.from_numpy(batch["rgb"]))
        depth.copy_(torch.from_numpy(batch["depth"]))

    def step():
        eng.encode(masks, offsets)
        eng.forward(bgr, depth, offsets, logits)
        eng.postprocess(logits, post)

    try:
        load(31)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        load(32)
        eng.set_option(24, 0)
        step()                             # one stream, eager: the reference
        torch.cuda.synchronize()
        eager = (logits.clone(), post["panoptic"].clone(), post["count"].clone())
        eng.set_option(24, 1)
        assert float(eager[0].abs().max()) > 1.0
        for _ in range(2):
            logits.zero_()
            post["panoptic"].zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(logits, eager[0]) and torch.equal(post["panoptic"], eager[1]) and torch.equal(post["count"], eager[2])
    finally:
        eng.close()


def test_winograd_modes_agree():
    """The convolution algorithms (direct only, Winograd F(2x2,3x3), F(4x4,3x3), F(6x6,3x3) forced on every layer it fits:
    quber_set_tuning keys 6 / 9, the C-level form of QUBER_WINOGRAD) give the same logits within the 1e-4 bar, and the library reports how many of the
    algorithmic FLOPs each one executes."""
    from quber_amd import _lib
    lib = _lib.load()
    h, w, b = 192, 256, 1      # 48 x 64 stride-4 maps: large enough for the 6x6 tiles to beat the 4x4 ones by >= 10 %
    sd = arch.init_state_dict(seed=6)
    batch, offs = inputs(9, b, h, w, 5)
    bgr, dep, off = torch.from_numpy(batch["rgb"]).cuda(), torch.from_numpy(batch["depth"]).cuda(), torch.from_numpy(offs).cuda()
    outs, ratios = {}, {}
    try:
        for name, (k6, k9) in {"off": (1, 0), "f2": (0, 2), "f4": (0, 4), "f6": (0, 6)}.items():
            lib.quber_set_tuning(6, k6)
            lib.quber_set_tuning(9, k9)
            eng = engine.Engine(engine.make_config(h, w, max_batch=b), "cuda:0")
            eng.load_state_dict(sd)
            outs[name] = eng.forward(bgr, dep, off).cpu()
            ratios[name] = eng.forward_flops_executed() / eng.forward_flops()
            del eng
    finally:
        lib.quber_set_tuning(6, 0)
        lib.quber_set_tuning(9, 0)
    assert ratios["off"] == 1.0 and ratios["f6"] < ratios["f4"] < ratios["f2"] < 1.0
    assert ratios["f4"] < 0.85 and ratios["f2"] < 0.9        # (only the stride-4 maps of this frame are large enough for the path)
    for name in ("f2", "f4", "f6"):
        assert float((outs[name] - outs["off"]).abs().max()) < TOL, name
    assert not torch.equal(outs["f4"], outs["off"])        # the path really was different


@pytest.mark.gpu
def test_launch_structures_agree():
    """One tile per block with separate projection shortcuts (tuning keys 13 = 0, 18 = 0) against the default plan
    (persistent launches, conv3 + shortcut as one dual-input GEMM) at a batch where both structures are active: the two
    are re-associations of the same fp32 sums (K shared between blocks; BN scales folded into the fused weights), so the
    head outputs agree inside the 1e-4 bar, with loud predictors, and the post-processed label maps coincide."""
    from quber_amd import _lib
    lib = _lib.load()
    h, w, b, n = 240, 320, 8, 10
    sd = arch.init_state_dict(seed=3, loud_heads=True, center_bias=-1.5)
    batch, offs = inputs(21, b, h, w, n)
    bgr, dep, off = torch.from_numpy(batch["rgb"]).cuda(), torch.from_numpy(batch["depth"]).cuda(), torch.from_numpy(offs).cuda()
    outs, pans, names = {}, {}, {}
    try:
        for name, (k13, k18) in {"old": (0, 0), "new": (1, 1)}.items():
            eng = engine.Engine(engine.make_config(h, w, max_batch=b, max_instances=n), "cuda:0")
            eng.set_option(13, k13)
            eng.set_option(18, k18)
            eng.load_state_dict(sd)
            lg = eng.forward(bgr, dep, off)
            pans[name] = eng.postprocess(lg)["panoptic"].cpu()
            outs[name] = lg.cpu()
            names[name] = [p[0] for p in eng.plan() if p[1] == "conv"]
            del eng
    finally:
        pass
    assert len(names["old"]) == len(names["new"]) + 4 and sum("+ shortcut" in s for s in names["new"]) == 4
    d = (outs["new"] - outs["old"]).abs()
    # (the oracle's own fp32 result sits 7e-5 from its float64 one on these O(1-10) logits; offset planes carry the stride factor 4)
    assert float(d[:, :2].max()) < TOL and float(d[:, 2:4].max()) < 4 * TOL and float(d[:, 4:].max()) < TOL
    assert not torch.equal(outs["new"], outs["old"])
    assert float((pans["new"] == pans["old"]).float().mean()) > 0.999


@pytest.mark.parametrize("h,w,b", [(256, 320, 2), (70, 102, 3)])
def test_stem_fused_fp16_data_path(h, w, b):
    """fp16 data path: a3 + stem.conv1 as one kernel on the fp16-rounded operands - csrc/stem.hip, its matrix-pipe form (key 29 = 1,
    default: v_mfma_f32_16x16x32_f16 on 16-byte LDS pixels) and its vector-FMA form (key 29 = 2) - against the preprocess kernel + fp16
    implicit GEMM (key 29 = 0).  All three multiply the same fp16 operands exactly and sum in fp32 - in different orders (the MFMA's
    internal tree) - so the stem output agrees to the last place of fp16 and the logits to the path's tolerance; the fused plans hold
    no 16-channel input tensor."""
    sd = arch.init_state_dict(seed=7, loud_heads=True, center_bias=-1.5)
    batch, offs = inputs(61, b, h, w, 4)
    bgr, dep, off = torch.from_numpy(batch["rgb"]).cuda(), torch.from_numpy(batch["depth"]).cuda(), torch.from_numpy(offs).cuda()
    outs = []
    for fused, dt in ((1, 2), (2, 2), (0, 2), (1, 0)):                  # the last: exact fp32, the yardstick for the logits
        qc = engine.make_config(h, w, max_batch=b)
        qc.compute_dtype = dt
        eng = engine.Engine(qc, "cuda:0")
        eng.set_option(29, fused)
        eng.load_state_dict(sd)
        outs.append((eng.forward(bgr, dep, off).clone(), eng.debug_tensor("stem1", b).float().clone()))
        eng.close()
    s0 = outs[2][1]
    e0 = float((outs[2][0] - outs[3][0]).abs().max())
    for form in (0, 1):
        s1 = outs[form][1]
        assert s1.shape == s0.shape and float(s0.abs().max()) > 0.1
        d = (s1 - s0).abs()
        assert float((d / (s0.abs() + 1e-2)).max()) < 2e-3             # one fp16 place (2^-10 relative)
        assert float((d > 0).float().mean()) < 0.02                      # and rarely that
        # a last-place flip in the stem travels through 80 fp16 layers: the forms are equally far from the fp32 network
        e1 = float((outs[form][0] - outs[3][0]).abs().max())
        assert e0 > 0 and e1 < 1.5 * e0 + 1e-3, (form, e1, e0)


@pytest.mark.parametrize("h,w,b,name", [(150, 203, 3, None), (96, 128, 2, "single-stream"), (256, 320, 2, "m-b-f-c-o-e2")],
                         ids=["ragged-default", "single-stream", "run_eval-default-yaml"])
def test_fp16_lean_loader_equals_tap_arithmetic(h, w, b, name):
    """fp16 data path (compute_dtype 2, configs[4] stand-in): the implicit GEMM with block-uniform filter taps, tap-validity masks and
    buffer loads (conv_igemm.hip LEAN, key 30 = 1) against the per-thread tap arithmetic (key 30 = 0): every convolution of the
    network (1x1, 3x3 with stride / dilation, 5x5 heads, padded borders) gives the same bits, so the logits do."""
    kw = VARIANTS[name] if name else {}
    qc = engine.set_arch(engine.make_config(h, w, max_batch=b), **kw)
    qc.compute_dtype = 2
    e = engine.Engine(qc, "cuda:0")
    e.load_state_dict(arch.init_state_dict(seed=11, loud_heads=True, **kw))
    batch, offs = inputs(5, b, h, w, 6)
    bgr, dep, off = torch.from_numpy(batch["rgb"]).cuda(), torch.from_numpy(batch["depth"]).cuda(), torch.from_numpy(offs).cuda()
    single = kw.get("streams", 2) == 1
    outs = {}
    e.set_option(31, 0)       # (the wide layers' 256 x 256-tile kernel, csrc/conv_h8.hip, has no tap-arithmetic form: tests/test_gpu_h8.py)
    for mode in (0, 1):
        e.set_option(30, mode)
        outs[mode] = e.forward(bgr, None if single else dep, off).clone()
    assert e.get_option(30) == 1
    assert torch.isfinite(outs[1]).all() and float(outs[1].abs().max()) > 0
    assert torch.equal(outs[0], outs[1])
    e.close()


def test_two_engines_keep_their_own_options():
    """Options belong to a context (quber_set_option), not to the process: two engines with different plan-time and
    arithmetic-changing settings live side by side, interleaved on one thread and concurrently on two, and each keeps producing
    exactly its own results; a later change of the process defaults (quber_set_tuning) touches neither."""
    import threading
    lib = _lib.load()
    h, w, b, n = 192, 256, 2, 6
    sd = arch.init_state_dict(seed=4, loud_heads=True, center_bias=-1.5)
    batch, offs = inputs(33, b, h, w, n)
    bgr, dep, off = torch.from_numpy(batch["rgb"]).cuda(), torch.from_numpy(batch["depth"]).cuda(), torch.from_numpy(offs).cuda()
    A = engine.Engine(engine.make_config(h, w, max_batch=b, max_instances=n), "cuda:0")
    B = engine.Engine(engine.make_config(h, w, max_batch=b, max_instances=n), "cuda:0")
    try:
        B.set_option(6, 1)            # plan: no Winograd layers at all
        B.set_option(18, 0)           # plan: projection shortcuts as convolutions of their own
        B.set_option(21, 0)           # arithmetic: one sequential fp32 chain over K
        B.set_option(24, 0)           # launch: no side lanes
        assert A.get_option(6) == 0 and A.get_option(21) == 2 and B.get_option(6) == 1 and B.get_option(21) == 0
        A.load_state_dict(sd)
        B.load_state_dict(sd)
        with pytest.raises(_lib.QuberError, match="before quber_finalize_weights"):
            A.set_option(25, 0)       # a plan-time key after the plan exists
        with pytest.raises(_lib.QuberError, match="unknown option"):
            A.set_option(99, 1)
        assert A.forward_flops_executed() < 0.9 * A.forward_flops() and B.forward_flops_executed() == B.forward_flops()
        assert sum("+ shortcut" in p[0] for p in A.plan()) == 4 and sum("+ shortcut" in p[0] for p in B.plan()) == 0
        a0, b0 = A.forward(bgr, dep, off).clone(), B.forward(bgr, dep, off).clone()
        assert not torch.equal(a0, b0)
        d = (a0 - b0).abs()
        assert float(d[:, :2].max()) < 2 * TOL and float(d[:, 4:].max()) < 2 * TOL      # two plans of the same network
        lib.quber_set_tuning(6, 1)    # process defaults: neither existing engine may notice
        lib.quber_set_tuning(21, 0)
        try:
            for _ in range(3):        # interleaved on one thread
                assert torch.equal(A.forward(bgr, dep, off), a0)
                assert torch.equal(B.forward(bgr, dep, off), b0)
        finally:
            lib.quber_set_tuning(6, 0)
            lib.quber_set_tuning(21, 2)
        # concurrently: one thread and one stream per engine
        bad = []

        def worker(eng, want):
            try:
                torch.cuda.set_device(0)
                st = torch.cuda.Stream()
                with torch.cuda.stream(st):
                    for _ in range(8):
                        got = eng.forward(bgr, dep, off)
                        st.synchronize()
                        if not torch.equal(got, want):
                            bad.append("mismatch")
            except Exception as e:      # noqa: BLE001
                bad.append(repr(e))

        torch.cuda.synchronize()
        ts = [threading.Thread(target=worker, args=(A, a0)), threading.Thread(target=worker, args=(B, b0))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not bad, bad
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("h,w,b", [(480, 640, 2), (70, 102, 3), (53, 75, 1)])
def test_stem_fused_equals_preprocess_plus_gemm(h, w, b):
    """a3 inside the first stem convolution's kernel (csrc/stem.hip, option key 29, default) against the preprocess kernel + implicit
    GEMM it replaces: the same fmaf chains in the same order (K-slices of the packed GEMM, two-level sums, fmaf epilogue), so the
    whole network's output is bit-identical - odd frame sizes (ragged last tiles, borders) included."""
    sd = arch.init_state_dict(seed=7, loud_heads=True, center_bias=-1.5)
    batch, offs = inputs(61, b, h, w, 4)
    bgr, dep, off = torch.from_numpy(batch["rgb"]).cuda(), torch.from_numpy(batch["depth"]).cuda(), torch.from_numpy(offs).cuda()
    outs, plans = [], []
    for fused in (1, 0):
        eng = engine.Engine(engine.make_config(h, w, max_batch=b), "cuda:0")
        eng.set_option(29, fused)
        eng.load_state_dict(sd)
        outs.append((eng.forward(bgr, dep, off).clone(), eng.debug_tensor("res2", b).clone()))
        plans.append(eng.plan())
        eng.close()
    first_conv = [next(op for op in pl if op[1] == "conv")[0] for pl in plans]      # (the plan opens with the GroupNorm-sum fill on a side lane)
    assert len(plans[0]) == len(plans[1]) and first_conv[0] == first_conv[1] == "backbone.rgb_backbone.stem.conv1"
    assert torch.equal(outs[0][1], outs[1][1]), "res2 differs"
    assert torch.equal(outs[0][0], outs[1][0]), "logits differ"
