"""GPU: the zoom-in refinement on the device (csrc/zoom.hip through Engine.zoom_rois / zoom_crop / zoom_paste and
MaskRefinerPredictor(zoom=...)) against its numpy contract (tests/test_zoom_cpu.py).  Integers and three float32 expressions: every
comparison is exact.  Every stage is held to the contract on the stage's OWN recorded inputs, so nothing here assumes that the network's
logits are invariant under the batch size."""
import ctypes as C

import numpy as np
import pytest
import torch

from quber_amd import engine
from quber_amd.eval.refiner_model import MaskRefiner
from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
from quber_amd.zoom import ZoomIn
from test_gpu_iterate import _case
from test_zoom_cpu import MAX_ID, hand_cases, overflow_case, overlap_np, pipeline_np, scene, zoom_crop_np, zoom_paste_np, zoom_rois_np

pytestmark = pytest.mark.gpu

SHAPES = [(9, 20), (33, 64), (70, 131)]                      # 180 pixels: less than a block; 16-byte rows; odd, several blocks
CROPS = [8, 33, 64]                                          # smaller than, coprime to / larger than the ROIs; 33: the byte paths
COUNTS = [0, 1, 7, 254]
FILL = 0x3C
_ES = {torch.uint8: 1, torch.int32: 4, torch.float32: 4}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_ENGINES = {}


def _engine(h, w, batch=3):
    key = (h, w, batch)
    if key not in _ENGINES:
        _ENGINES[key] = engine.Engine(engine.make_config(h, w, max_batch=batch, max_instances=64, with_network=False), "cuda:0")
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    torch.cuda.synchronize()
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


class Arena:
    """Device tensors `shift` elements (16: sixteen BYTES) into allocations filled with a sentinel byte."""

    def __init__(self, shift):
        self.shift, self.raw = shift, []

    def empty(self, shape, dtype):
        es = _ES[dtype]
        off = 16 if self.shift == 16 else self.shift * es
        n = int(np.prod(shape)) * es
        raw = torch.full((off + n + 64,), FILL, dtype=torch.uint8, device="cuda")
        self.raw.append((raw, off, n))
        return raw[off:off + n].view(dtype).view(tuple(shape))

    def put(self, a):
        t = self.empty(a.shape, {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32,
                                 np.dtype(np.uint32): torch.int32}[a.dtype])
        t.copy_(dev(a.view(np.int32) if a.dtype == np.uint32 else a))
        return t

    def intact(self):
        return all(bool((raw[:off] == FILL).all()) and bool((raw[off + n:] == FILL).all()) for raw, off, n in self.raw)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want.astype(got.dtype)), err_msg=what)


def _stages(eng, p, shift, what, outs=None):
    """The three entries on the inputs the contract `p` recorded for each stage, into guarded outputs -> the outputs (for a second call)."""
    B, (h, w) = len(p["ids"]), p["ids"].shape[1:]
    a = Arena(shift)
    n, T, S, N = p["n_ids"], len(p["slots"]), p["S"], p["max_inst"]
    host = {k: p[k] for k in ("ids", "bgr", "depth", "slots", "rois", "crop_ids", "crop_scores", "table", "area", "depth_crop") if p[k] is not None}
    d = {k: a.put(v) for k, v in host.items()}
    if outs is None:
        outs = {"rois": a.empty((B, n, 4), torch.int32), "bc": a.empty((T, S, S, 3), torch.uint8), "mc": a.empty((T, 1, S, S), torch.uint8),
                "dc": a.empty((T, S, S, 3), torch.uint8) if "depth" in d else None,
                "final": {"ids": a.empty((B, h, w), torch.int32), "masks": a.empty((B, N, h, w), torch.uint8), "source": a.empty((B, N, 2), torch.int32),
                          "scores": a.empty((B, N), torch.float32), "boxes": a.empty((B, N, 4), torch.float32), "report": a.empty((B, 4), torch.int32)},
                "arena": a}
    r = eng.zoom_rois(d["ids"], n, p["padding"], outs["rois"])
    eng.zoom_crop(d["bgr"], d.get("depth"), d["ids"], d["slots"], d["rois"], S, (outs["bc"], outs["dc"], outs["mc"]))
    f = eng.zoom_paste(d.get("crop_ids"), d.get("crop_scores"), d.get("table"), d.get("area"), d.get("depth_crop"), d["slots"], d["rois"], B,
                       p["min_overlap"], N, outs["final"])
    torch.cuda.synchronize()
    assert a.intact() and outs["arena"].intact(), what + ": wrote outside a tensor"
    for k, v in host.items():
        _check(d[k], v.view(np.int32) if v.dtype == np.uint32 else v, what + ": the input %s changed" % k)
    if n:
        _check(r, p["rois"], what + " rois")
    if T:
        _check(outs["bc"], p["bgr_crop"], what + " bgr_crop")
        _check(outs["mc"], p["mask_crop"], what + " mask_crop")
        if "depth" in d:
            _check(outs["dc"], p["depth_crop"], what + " depth_crop")
    for k in ("ids", "masks", "source", "scores", "boxes", "report"):
        _check(f[k], p["final"][k], what + " final " + k)
    return outs


_CASES = {}


def _scene_case(h, w, n, S, B=1, with_depth=True):
    key = (h, w, n, S, B, with_depth)
    if key not in _CASES:
        ids, bgr, depth = scene(h, w, n, 1000 + 7 * n + S, B=B, with_depth=with_depth)
        _CASES[key] = pipeline_np(ids, n, bgr, depth, S, seed=n + S)
    return _CASES[key]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("S", CROPS)
@pytest.mark.parametrize("h,w", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_kernels_equal_contract(h, w, S, n):
    p = _scene_case(h, w, n, S)
    eng = _engine(h, w)
    for shift in (16, 1):                                    # 16 bytes in: the 16-byte paths where the shape allows them; 1 element in
        _stages(eng, p, shift, "%dx%d S=%d n=%d shift %d" % (h, w, S, n, shift))
    if n:
        assert p["final"]["report"][0, 3] >= 1
    if n == 254:
        assert (p["rois"][0, :, 2] < 0).any() or h * w > 254     # ids without a pixel ride along


@pytest.mark.parametrize("name", ["one_pixel", "touches_all_edges", "padding_ties", "absent_id", "equal_keys", "nothing_kept", "painted_over"])
def test_hand_cases_on_the_device(name):
    p = hand_cases()[name]
    for shift in (16, 1):
        _stages(_engine(33, 64), p, shift, name)


def test_overflow_past_254_on_the_device():
    p = overflow_case()
    assert p["final"]["report"][0].tolist() == [20, 320, 66, 254]
    _stages(_engine(70, 131), p, 16, "overflow")
    _stages(_engine(70, 131), overflow_case(max_inst=100), 1, "overflow at max_inst 100")


def test_no_depth_orders_by_roi_area():
    p = _scene_case(70, 131, 7, 33, with_depth=False)
    assert p["depth_crop"] is None
    _stages(_engine(70, 131), p, 16, "single stream")


def test_three_frames_with_different_counts_then_other_data_overwrites():
    h, w, S = 70, 131, 33
    ids, bgr, depth = scene(h, w, 7, 77, B=3)
    ids[1][ids[1] > 3] = 0
    ids[2][:] = 0
    slots = np.array([(b, j) for b, k in enumerate((7, 3, 0)) for j in range(1, k + 1)], np.int32)
    p = pipeline_np(ids, 7, bgr, depth, S, slots=slots, seed=5)
    assert [int(c) for c in p["final"]["report"][:, 0]] == [7, 3, 0] and p["final"]["report"][2].tolist() == [0, 0, 0, 0]
    eng = _engine(h, w)
    outs = _stages(eng, p, 16, "three frames")
    ids2, bgr2, depth2 = scene(h, w, 7, 78, B=3)
    q = pipeline_np(ids2, 7, bgr2, depth2, S, seed=6)        # the same shapes but for the slots: 21 crops
    outs2 = _stages(eng, q, 16, "other data")
    # and into the SAME output tensors a call with fewer instances leaves nothing of the previous one behind
    small = pipeline_np(ids, 7, bgr, depth, S, slots=slots, seed=5)
    d = {k: dev(small[k].view(np.int32) if small[k].dtype == np.uint32 else small[k]) for k in
         ("crop_ids", "crop_scores", "table", "area", "depth_crop", "slots", "rois")}
    f = eng.zoom_paste(d["crop_ids"], d["crop_scores"], d["table"], d["area"], d["depth_crop"], d["slots"], d["rois"], 3, 0.5, MAX_ID, outs2["final"])
    torch.cuda.synchronize()
    for k in ("ids", "masks", "source", "scores", "boxes", "report"):
        _check(f[k], small["final"][k], "overwrite " + k)
    assert outs is not outs2


def test_bad_arguments_are_refused_and_launch_nothing():
    h, w = 33, 64
    p = _scene_case(h, w, 7, 8)
    eng = _engine(h, w)
    a = Arena(16)
    d = {k: a.put(p[k].view(np.int32) if p[k].dtype == np.uint32 else p[k]) for k in
         ("ids", "bgr", "depth", "slots", "rois", "crop_ids", "crop_scores", "table", "area", "depth_crop")}
    rois = a.empty((1, 7, 4), torch.int32)
    lib, P = eng.lib, lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"ids": a.empty((1, h, w), torch.int32), "masks": a.empty((1, 8, h, w), torch.uint8), "source": a.empty((1, 8, 2), torch.int32),
           "scores": a.empty((1, 8), torch.float32), "boxes": a.empty((1, 8, 4), torch.float32), "report": a.empty((1, 4), torch.int32)}
    bc, mc = a.empty((7, 8, 8, 3), torch.uint8), a.empty((7, 1, 8, 8), torch.uint8)

    def paste(**kw):
        v = dict(T=7, S=8, Cn=3, mo=0.5, N=8, B=1, n=7, ids=P(out["ids"]))
        v.update(kw)
        return lib.quber_zoom_paste(eng.h, P(d["crop_ids"]), P(d["crop_scores"]), P(d["table"]), P(d["area"]), P(d["depth_crop"]), P(d["slots"]),
                                    P(d["rois"]), v["B"], v["n"], v["T"], v["S"], v["Cn"], v["mo"], v["N"], v["ids"], P(out["masks"]),
                                    P(out["source"]), P(out["scores"]), P(out["boxes"]), P(out["report"]), st)

    def crop(**kw):
        v = dict(T=7, S=8, B=1, n=7, bc=P(bc))
        v.update(kw)
        return lib.quber_zoom_crop(eng.h, P(d["bgr"]), P(d["depth"]), P(d["ids"]), P(d["slots"]), P(d["rois"]), v["B"], v["n"], v["T"], v["S"],
                                   v["bc"], P(bc), P(mc), st)

    bad = [lambda: lib.quber_zoom_rois(eng.h, P(d["ids"]), 1, 255, 0.25, P(rois), st),
           lambda: lib.quber_zoom_rois(eng.h, P(d["ids"]), 4, 7, 0.25, P(rois), st),
           lambda: lib.quber_zoom_rois(eng.h, P(d["ids"]), 1, 7, float("nan"), P(rois), st),
           lambda: lib.quber_zoom_rois(eng.h, P(d["ids"]), 1, 7, -0.5, P(rois), st),
           lambda: lib.quber_zoom_rois(eng.h, C.c_void_p(0), 1, 7, 0.25, P(rois), st),
           lambda: lib.quber_zoom_rois(eng.h, P(d["ids"]), 1, 7, 0.25, C.c_void_p(rois.data_ptr() + 1), st),
           lambda: crop(S=1), lambda: crop(S=513), lambda: crop(n=255), lambda: crop(B=0), lambda: crop(T=3 * 254 + 1), lambda: crop(bc=C.c_void_p(0)),
           lambda: paste(S=1), lambda: paste(S=513), lambda: paste(Cn=0), lambda: paste(Cn=255), lambda: paste(N=0), lambda: paste(N=255),
           lambda: paste(mo=float("nan")), lambda: paste(B=4), lambda: paste(n=-1), lambda: paste(T=-1), lambda: paste(ids=C.c_void_p(0)),
           lambda: paste(ids=C.c_void_p(out["ids"].data_ptr() + 2))]
    for k, f in enumerate(bad):
        assert f() != 0, "bad call %d was accepted" % k
        assert lib.quber_last_error().decode(), k
    torch.cuda.synchronize()
    assert a.intact()
    for t in list(out.values()) + [rois, bc, mc]:
        assert bool((t.view(torch.uint8) == FILL).all()), "a refused call wrote an output"
    assert paste() == 0 and crop() == 0                      # and the same arguments, valid, are accepted
    torch.cuda.synchronize()


# ---- predictor level ---------------------------------------------------------------------------------------------------------------------
H, W, NM, CROP = 192, 256, 6, 128


def _hold_to_contract(rec, outs, zoom, two=True):
    """One debug_zoom record (every tensor on the host) against the contract on the record's own inputs, and the dicts against its tables."""
    ids, slots, rois = rec["ids"], rec["slots"], rec["rois"]
    B, n = len(ids), rois.shape[1]
    np.testing.assert_array_equal(rois, zoom_rois_np(ids, n, zoom.padding))
    bc, dc, mc = zoom_crop_np(rec["bgr"], rec["depth"], ids, slots, rois, zoom.crop)
    np.testing.assert_array_equal(rec["bgr_crop"], bc)
    np.testing.assert_array_equal(rec["mask_crop"], mc)
    assert (rec["depth"] is not None) == two
    if two:
        np.testing.assert_array_equal(rec["depth_crop"], dc)
    Cn = rec["crop_scores"].shape[1]
    table, area = overlap_np(rec["mask_crop"], rec["crop_ids"], Cn)
    np.testing.assert_array_equal(rec["table"], table.astype(np.int32))
    np.testing.assert_array_equal(rec["area"], area.astype(np.int32))
    N = rec["final"]["masks"].shape[1]
    want = zoom_paste_np(rec["crop_ids"], rec["crop_scores"], table, area, rec["depth_crop"], slots, rois, B, ids.shape[1], ids.shape[2],
                         zoom.min_overlap, N)
    for k in ("ids", "masks", "source", "scores", "boxes", "report"):
        np.testing.assert_array_equal(_bits(rec["final"][k]), _bits(want[k]), err_msg=k)
    for b, o in enumerate(outs):
        crops, kept, dropped, count = (int(v) for v in want["report"][b])
        assert o["zoom_report"].tolist() == [crops, kept, dropped, count]
        np.testing.assert_array_equal(o["zoom_ids"].cpu().numpy(), want["ids"][b])
        np.testing.assert_array_equal(o["zoom_rois"].cpu().numpy(), rois[b, :crops])
        k1 = len(o["coarse_instances"]) if "coarse_instances" in o else 0
        assert crops == k1 and "sem_seg" in o and "panoptic_seg" in o
        if count:
            inst = o["instances"]
            np.testing.assert_array_equal(inst.pred_masks.cpu().numpy(), want["masks"][b, :count] != 0)
            np.testing.assert_array_equal(_bits(inst.scores.cpu().numpy()), _bits(want["scores"][b, :count]))
            np.testing.assert_array_equal(inst.pred_boxes.tensor.cpu().numpy(), want["boxes"][b, :count])
            np.testing.assert_array_equal(inst.zoom_source.cpu().numpy(), want["source"][b, :count])
            assert not inst.pred_classes.cpu().numpy().any() and len(inst) == count
        else:
            assert "instances" not in o
    return want


_HOST = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else {k: _HOST(x) for k, x in v.items()} if isinstance(v, dict) else v

RGB_ONLY = ("MODEL:\n  META_ARCHITECTURE: MaskRefiner\n  BACKBONE:\n    NAME: build_resnet_deeplab_fusion_backbone\n"
            "  RESNETS:\n    OUT_FEATURES: [res2, res3, res5]\n    RES5_DILATION: 2\n"
            "  PIXEL_MEAN: [103.53, 116.28, 123.675]\n  PIXEL_STD: [1, 1, 1]\n"
            "  INS_EMBED_HEAD:\n    NAME: MaskRefinerInsEmbedHead\n    NORM: GN\n    HIERARCHICAL_FUSION_ON: True\n"
            "    EEE_BOUNDARY_ON: True\n    HIERARCHY: [[eee_boundary], [foreground, center, offset]]\n"
            "    FUSION_TARGET: [feat, pred]\n    ERROR_TYPE: e3\n"
            "  PANOPTIC_DEEPLAB:\n    CENTER_THRESHOLD: 0.3\n    STUFF_AREA: 2048\nINPUT:\n  OFFSET_INPUT_ON: True\n  DEPTH_ON: False\n  RGB_ON: True\n")


def _predict(zoom, counts=(NM,), batched=False, config=None, sd=None, **kw):
    """predict (or predict_batch) of len(counts) seeded frames with counts[b] initial masks each -> (dicts, debug_zoom records on the host)."""
    batch, sd_loud, _ = _case(H, W, len(counts), NM)
    masks = [batch["masks"][b][:c] for b, c in enumerate(counts)]
    pred = MaskRefinerPredictor(config, device="cuda:0", state_dict=sd_loud if sd is None else sd, zoom=zoom, **kw)
    pred.model.debug_zoom = []
    try:
        if batched:
            outs = pred.predict_batch(batch["rgb"], batch["depth"], masks)
        else:
            outs = pred.predict(batch["rgb"][0], batch["depth"][0], masks[0])
        torch.cuda.synchronize()
        recs = [_HOST(r) for r in pred.model.debug_zoom]
        assert (pred.model._zoom_model is not None) == (len(recs[0]["slots"]) > 0)
    finally:
        pred.model.close()
    assert pred.model._zoom_model is None
    return outs, recs


@pytest.mark.parametrize("tta", [False, True], ids=["plain", "tta"])
def test_predict_holds_every_stage_to_the_contract(tta):
    zoom = ZoomIn(crop=CROP)
    outs, recs = _predict(zoom, tta=tta)
    assert len(outs) == 1 and len(recs) == 1
    want = _hold_to_contract(recs[0], outs, zoom)
    print("zoomed predict tta=%s: report (crops, kept, dropped, count) = %s" % (tta, want["report"][0].tolist()))
    assert want["report"][0, 0] >= 1, "the seeded case produced no first-pass instance: nothing was zoomed"


def test_predict_batch_three_frames_of_different_counts():
    zoom = ZoomIn(crop=CROP, batch=4)                        # several chunks of crops, the last one short
    outs, recs = _predict(zoom, counts=(NM, 2, 0), batched=True)
    assert len(outs) == 3 and len(recs) == 1
    want = _hold_to_contract(recs[0], outs, zoom)
    print("zoomed predict_batch: reports = %s" % want["report"].tolist())
    assert want["report"][:, 0].sum() >= 2


def test_single_stream_orders_by_roi_area(tmp_path):
    from quber_amd import arch
    cfg = tmp_path / "rgb_only.yaml"
    cfg.write_text(RGB_ONLY)
    zoom = ZoomIn(crop=CROP)
    outs, recs = _predict(zoom, config=str(cfg), sd=arch.init_state_dict(seed=2, loud_heads=True, center_bias=-1.68, streams=1))
    assert recs[0]["depth"] is None and recs[0]["depth_crop"] is None
    want = _hold_to_contract(recs[0], outs, zoom, two=False)
    print("zoomed single-stream predict: report = %s" % want["report"][0].tolist())
    assert want["report"][0, 0] >= 1, "no first-pass instance: nothing was zoomed"


def test_zoom_none_changes_nothing_and_stream_refuses():
    batch, sd, _ = _case(H, W, 1, NM)
    bgr, depth, masks = batch["rgb"][0], batch["depth"][0], batch["masks"][0]
    a = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd)
    b = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, zoom=None)
    try:
        ra, rb = a.predict(bgr, depth, masks)[0], b.predict(bgr, depth, masks)[0]
        assert list(ra) == list(rb) and "instances" in ra and b.model.zoom is None and b.model._zoom_model is None
        for k in ra:
            if k == "instances":
                assert sorted(ra[k].get_fields()) == sorted(rb[k].get_fields())
                for f in ra[k].get_fields():
                    x, y = ra[k].get(f), rb[k].get(f)
                    x, y = (x.tensor, y.tensor) if hasattr(x, "tensor") else (x, y)
                    assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), f
            else:
                x, y = (ra[k][0], rb[k][0]) if isinstance(ra[k], tuple) else (ra[k], rb[k])
                assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), k
    finally:
        a.model.close()
        b.model.close()
    with pytest.raises(ValueError, match="zoom"):
        MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, zoom="yes")
    with pytest.raises(ValueError, match="512"):
        ZoomIn(crop=513)
    m = MaskRefiner(zoom=ZoomIn(crop=CROP))
    try:
        with pytest.raises(ValueError, match="zoom"):
            next(iter(m.predict_stream([("a.png", "b.png", masks)], batch=2)))
        with pytest.raises(ValueError, match="zoom"):
            m.refiner_predictor.model.enqueue_batch(dev(bgr[None]), dev(depth[None]), dev(masks[None]))
    finally:
        m.refiner_predictor.model.close()


def test_adapter_round_trip(tmp_path):
    from PIL import Image
    batch, sd, _ = _case(480, 640, 1, 8)
    Image.fromarray(batch["rgb"][0][:, :, ::-1].copy()).save(tmp_path / "rgb.png")
    Image.fromarray(batch["depth"][0][:, :, 0].astype(np.uint16) * 5 + 300).save(tmp_path / "depth.png")
    zoom = ZoomIn(crop=CROP)
    m = MaskRefiner(None, weights_file=None, dataset="OSD", zoom=zoom)
    model = m.refiner_predictor.model
    model.state_dict = sd
    model.debug_zoom = []
    try:
        refined, output, seconds, fg = m.predict(str(tmp_path / "rgb.png"), str(tmp_path / "depth.png"), batch["masks"][0] != 0)
        torch.cuda.synchronize()
        recs = [_HOST(r) for r in model.debug_zoom]
    finally:
        model.close()
    want = _hold_to_contract(recs[0], [output], zoom)
    count = int(want["report"][0, 3])
    print("zoomed adapter predict: report = %s" % want["report"][0].tolist())
    assert want["report"][0, 0] >= 1 and len(refined) == count and seconds > 0
    if count:
        np.testing.assert_array_equal(np.asarray(refined), want["masks"][0, :count] != 0)
