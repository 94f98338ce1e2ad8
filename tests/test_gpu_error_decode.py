"""GPU: the predicted error maps on the device (INTEGRATION.md "Predicted error maps"; csrc/errhead.hip).

The four kernels against the numpy statements of tests/test_error_decode_cpu.py (all integer results exactly), the decoded classes
of loud heads against torch.argmax of the same logits and against the CPU oracle network's argmax, the predictor paths with
decode_errors on and off, the adapter's scoring / visualisation, and the decode -> attribute -> score chain as one hipGraph."""
import numpy as np
import pytest
import torch

from oracle import errmaps_np
from quber_amd import engine, synth
from quber_amd.eval import error_maps as em
from test_error_decode_cpu import confusion_np, decode_np, mask_hist_np, overlay_np
from test_gpu_loud_parity import _oracle, _scene, loud_state_dict
from test_gpu_tta import MASK_KW

pytestmark = pytest.mark.gpu

GUARD = 0x3C


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bare_engine(h, w, b, n=1):
    return engine.Engine(engine.make_config(h, w, max_batch=b, max_instances=max(n, 1), with_network=False), "cuda:0")


def shifted(shape, dtype, shift_elems, fill=None):
    """A tensor of `shape` that starts `shift_elems` elements into a guard-filled allocation -> (allocation as bytes, tensor)."""
    n = int(np.prod(shape))
    es = torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((n + shift_elems) * es + 64,), GUARD, dtype=torch.uint8, device="cuda")
    t = raw[shift_elems * es:(shift_elems + n) * es].view(dtype).view(shape)
    if fill is not None:
        t.copy_(fill)
    return raw, t


def guards_intact(raw, t):
    lo = t.data_ptr() - raw.data_ptr()
    hi = lo + t.numel() * t.element_size()
    return bool((raw[:lo] == GUARD).all()) and bool((raw[hi:] == GUARD).all())


def tie_logits(shape, seed):
    """Logits from a handful of values: ties everywhere, +-0.0, +-inf and NaN among them (1 / 16 of the elements each)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    table = torch.tensor([0.0, -0.0, 1.0, 1.0, -1.0, 0.5, 0.5, 2.0, 2.0, -2.0, 0.0, 1.0, float("inf"), float("-inf"), float("nan"), -0.0],
                         dtype=torch.float32, device="cuda")
    return table[torch.randint(0, 16, shape, generator=g, device="cuda")].contiguous()


# ---- 1. decode ----
@pytest.mark.parametrize("h,w,b,shift", [(96, 241, 1, 0), (48, 97, 1, 7), (64, 128, 2, 0), (480, 640, 16, 0)],
                         ids=["96x241", "48x97-shift7", "64x128-b2", "480x640-b16"])
def test_decode_equals_torch_argmax(h, w, b, shift):
    """shift: the class map starts 7 bytes, the logits 7 floats (28 bytes), the histogram 1 word into their allocations - no plane, row
    or output is 16-byte aligned; nothing outside the outputs is written."""
    eng = bare_engine(h, w, b)
    for classes in (2, 3, 4):
        planes = 4 + 2 * classes
        lraw, lg = shifted((b, planes, h, w), torch.float32, shift, tie_logits((b, planes, h, w), h * w + classes))
        host = lg.cpu()
        assert bool(torch.isnan(host).any()) and bool(torch.isinf(host).any())
        for first in (4, 4 + classes):
            craw, cls = shifted((b, h, w), torch.uint8, shift)
            hraw, hist = shifted((b, classes), torch.int32, 1 if shift else 0)
            eng.error_decode(lg, (first, classes), cls, hist)
            want = torch.argmax(host[:, first:first + classes], dim=1)
            assert torch.equal(cls.cpu().long(), want), (classes, first)
            want_hist = torch.stack([torch.bincount(x.reshape(-1), minlength=classes) for x in want])
            assert torch.equal(hist.cpu().long(), want_hist), (classes, first)
            assert guards_intact(craw, cls) and guards_intact(hraw, hist)
            # a second call into the same buffers: overwritten, not accumulated
            eng.error_decode(lg, (first, classes), cls, hist)
            assert torch.equal(cls.cpu().long(), want) and torch.equal(hist.cpu().long(), want_hist)
            assert guards_intact(craw, cls) and guards_intact(hraw, hist)
        # the raw entry with dev_hist = NULL
        out = torch.full((b, h, w), 9, dtype=torch.uint8, device="cuda")
        assert eng.lib.quber_error_decode(eng.h, lg.data_ptr(), planes, 4, classes, b, out.data_ptr(), None, engine._stream()) == 0
        assert torch.equal(out.cpu().long(), torch.argmax(host[:, 4:4 + classes], dim=1))
        del lraw
    with pytest.raises(engine._lib.QuberError):              # planes beyond the logits are refused, not read
        engine._lib.check(eng.lib.quber_error_decode(eng.h, lg.data_ptr(), planes, planes - 1, 4, b, out.data_ptr(), None,
                                                     engine._stream()))
    eng.close()


def test_decode_np_statement_matches_the_kernel():
    h, w, b = 32, 48, 2
    eng = bare_engine(h, w, b)
    lg = tie_logits((b, 12, h, w), 5)
    cls, hist = eng.error_decode(lg, (8, 4))
    c_np, h_np = decode_np(lg.cpu().numpy(), 8, 4)
    assert np.array_equal(cls.cpu().numpy(), c_np) and np.array_equal(hist.cpu().numpy(), h_np)
    eng.close()


# ---- 2. mask histogram ----
def random_masks(rng, b, n, h, w):
    """Overlapping rectangles with bytes 1 or 255; mask 1 of every frame (if there is one) is empty."""
    m = np.zeros((b, n, h, w), np.uint8)
    for i in range(b):
        for j in range(n):
            if j == 1:
                continue
            y0, x0 = rng.integers(0, h - 4), rng.integers(0, w - 4)
            y1, x1 = rng.integers(y0 + 1, h + 1), rng.integers(x0 + 1, w + 1)
            m[i, j, y0:y1, x0:x1] = 255 if j % 2 else 1
    return m


@pytest.mark.parametrize("h,w,b,shift", [(96, 241, 1, 0), (50, 97, 1, 0), (64, 128, 2, 0), (64, 128, 2, 7), (480, 640, 2, 0)],
                         ids=["96x241", "50x97-ragged", "64x128-b2", "64x128-b2-shift7", "480x640-b2"])
def test_mask_hist_equals_numpy(h, w, b, shift):
    """The small frames run one mask per block (the masks are split over blockIdx.z until the device is full), 480x640 several - with a
    short last chunk at N = 20, 37, 300."""
    rng = np.random.default_rng(h * w + shift)
    eng = bare_engine(h, w, b, 300)
    for n in (0, 1, 20, 37, 300):
        for classes in ((2, 3, 4) if n == 20 else (4,)):
            cls_np = rng.integers(0, classes, (b, h, w), dtype=np.uint8)
            m_np = random_masks(rng, b, n, h, w)
            craw, cls = shifted((b, h, w), torch.uint8, shift, dev(cls_np))
            mraw, masks = shifted((b, n, h, w), torch.uint8, shift, dev(m_np))
            oraw, out = shifted((b, n, classes), torch.int32, 1 if shift else 0)
            for _ in range(2):                          # the second call overwrites
                eng.error_mask_hist(cls, masks, classes, out)
                assert np.array_equal(out.cpu().numpy(), mask_hist_np(cls_np, m_np, classes)), (n, classes)
                assert guards_intact(oraw, out)
            if n > 1:
                assert int(out[:, 1].abs().sum()) == 0 and int(out.sum()) > 0          # the empty mask; the others are not
    # a class value outside the head's range is counted nowhere
    cls_np = rng.integers(0, 6, (b, h, w), dtype=np.uint8)
    m_np = random_masks(rng, b, 5, h, w)
    got = eng.error_mask_hist(dev(cls_np), dev(m_np), 4).cpu().numpy()
    assert np.array_equal(got, mask_hist_np(cls_np, m_np, 4))
    with pytest.raises(engine._lib.QuberError):
        eng.error_mask_hist(dev(cls_np), dev(random_masks(rng, b, 301, h, w)), 4)       # above max_instances
    eng.close()


# ---- 3. confusion table ----
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shift1"])
def test_score_equals_numpy(shift):
    h, w, b = 96, 128, 2
    rng = np.random.default_rng(3 + shift)
    eng = bare_engine(h, w, b, 6)
    init = np.stack([synth.make_scene(s, h, w, 5)["masks"] for s in (1, 2)])
    gt = np.stack([synth.make_scene(s, h, w, 4)["masks"] for s in (7, 8)])
    init, gt = (init != 0).astype(np.uint8), (gt != 0).astype(np.uint8)
    explicit = eng.error_maps(dev(init), dev(gt))
    ex_np = explicit.cpu().numpy()
    assert np.array_equal(ex_np, np.stack([errmaps_np.explicit_error_maps(init[i], gt[i]) for i in range(b)]))
    for et in em.ERROR_TYPES:
        C = em.n_classes(et)
        for kind in (0, 1):
            cls_np = rng.integers(0, C, (b, h, w), dtype=np.uint8)
            craw, cls = shifted((b, h, w), torch.uint8, shift, dev(cls_np))
            table = eng.error_score(cls, explicit, ("region", "boundary")[kind], et)
            eng.error_score(cls, explicit, kind, em.ERROR_TYPES.index(et), table)          # again, into the same table
            t = table.cpu().numpy()
            assert t.shape == (b, C + 1, C) and np.array_equal(t, confusion_np(cls_np, ex_np, kind, et)), (et, kind)
            assert t.sum((1, 2)).tolist() == [h * w] * b
            tptn = ex_np[:, kind, 0].astype(np.int64).sum((1, 2)) + ex_np[:, kind, 1].sum((1, 2))
            assert t[:, C].sum(1).tolist() == (tptn.tolist() if et == "e32" else [0] * b)
    # a predicted class outside the head's range is counted nowhere
    cls_np = rng.integers(0, 6, (b, h, w), dtype=np.uint8)
    t = eng.error_score(dev(cls_np), explicit, 1, "e3").cpu().numpy()
    assert np.array_equal(t, confusion_np(cls_np, ex_np, 1, "e3")) and int(t.sum()) == int((cls_np < 4).sum())
    with pytest.raises(engine._lib.QuberError):             # classes must match the error type
        engine._lib.check(eng.lib.quber_error_score(eng.h, dev(cls_np).data_ptr(), explicit.data_ptr(), 1, 1, 4, b,
                                                    torch.zeros(40, dtype=torch.int64, device="cuda").data_ptr(), engine._stream()))
    eng.close()


# ---- 4. overlay ----
@pytest.mark.parametrize("h,w,b,shift", [(50, 97, 2, 0), (50, 97, 2, 7), (64, 128, 1, 0)], ids=["50x97-b2", "50x97-b2-shift7", "64x128"])
def test_overlay_equals_numpy(h, w, b, shift):
    rng = np.random.default_rng(h + shift)
    eng = bare_engine(h, w, b)
    bgr_np = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    cls_np = rng.integers(0, 5, (b, h, w), dtype=np.uint8)          # class 4: never painted
    for palette in (em.DEFAULT_PALETTE["e3"], em.DEFAULT_PALETTE["e2"], ((1, 2, 3), (4, 5, 6), (7, 8, 9), (250, 251, 252)), ()):
        want = overlay_np(bgr_np, cls_np, palette)
        braw, bgr = shifted((b, h, w, 3), torch.uint8, shift, dev(bgr_np))
        craw, cls = shifted((b, h, w), torch.uint8, shift, dev(cls_np))
        oraw, out = shifted((b, h, w, 3), torch.uint8, shift)
        eng.error_overlay(bgr, cls, palette, out)                    # out of place
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(bgr.cpu().numpy(), bgr_np)
        assert guards_intact(oraw, out)
        eng.error_overlay(bgr, cls, palette, bgr)                    # in place
        assert np.array_equal(bgr.cpu().numpy(), want) and guards_intact(braw, bgr)
    eng.close()


def test_stage_profile_reports_the_four_stages():
    """quber_profile_begin / _end: one stage per kernel, with the algorithmic bytes computed from the shapes."""
    h, w, b, n = 64, 128, 2, 5
    eng = bare_engine(h, w, b, n)
    rng = np.random.default_rng(0)
    masks = dev(random_masks(rng, b, n, h, w))
    lg = tie_logits((b, 8, h, w), 1)
    bgr = dev(rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8))
    explicit = eng.error_maps(masks, masks)
    eng.profile_begin()
    cls, _ = eng.error_decode(lg, (4, 4))
    eng.error_mask_hist(cls, masks, 4)
    eng.error_score(cls, explicit, "boundary", "e3")
    eng.error_overlay(bgr, cls, em.DEFAULT_PALETTE["e3"])
    st = eng.profile_end()
    hw = b * h * w
    want = {"error_decode": 17 * hw, "error_mask_hist": hw * (n + 1) + 4 * b * n * 4, "error_score": 5 * hw + 8 * b * 20, "error_overlay": 7 * hw}
    for name, nbytes in want.items():
        assert name in st and st[name]["launches"] == 1 and st[name]["bytes"] == nbytes and st[name]["ms"] > 0, (name, st.get(name))
    eng.close()


# ---- 5. end to end, loud heads, against the CPU oracle ----
E2E = {"canonical": {}, "mask+boundary": MASK_KW, "e2": dict(error_classes=2), "e33": dict(error_classes=3),
       "mask+boundary-e2": dict(MASK_KW, error_classes=2)}
MARGIN = 2e-4          # each of the two leading logits may move by the suite's 1e-4 head bar
EXCUSED_CAP = 1e-3     # share of a frame's pixels that may differ from the oracle's argmax under that margin


@pytest.mark.parametrize("name", list(E2E), ids=list(E2E))
def test_decoded_classes_against_oracle(name):
    kw = E2E[name]
    h, w, b, n = 96, 128, 2, 3
    batch, offs, image = _scene(3, b, h, w, n)
    sd = loud_state_dict(1, image, offs, n, **kw)
    with torch.no_grad():
        ref = _oracle(sd, **kw)(image, torch.from_numpy(offs))
    eng = engine.Engine(engine.set_arch(engine.make_config(h, w, max_batch=b, max_instances=n), **kw), "cuda:0")
    eng.load_state_dict(sd)
    logits = eng.forward(dev(batch["rgb"]), dev(batch["depth"]), eng.encode(dev(batch["masks"])))
    heads = eng.error_heads()
    assert list(heads) == (["eee_boundary", "eee_mask"] if kw.get("eee_mask_on") else ["eee_boundary"])
    ncls = kw.get("error_classes", 4)
    o = 4
    for head, (first, classes) in heads.items():
        assert (first, classes) == (o, ncls)
        o += ncls
        cls, hist = eng.error_decode(logits, head)
        mine = torch.argmax(logits[:, first:first + classes], dim=1).cpu()
        assert torch.equal(cls.cpu().long(), mine)                                        # (a)
        assert torch.equal(hist.cpu().long(), torch.stack([torch.bincount(x.reshape(-1), minlength=classes) for x in mine]))
        r = ref[head]                                                                     # (b)
        want = torch.argmax(r, dim=1)
        top2 = torch.topk(r, 2, dim=1).values
        margin = top2[:, 0] - top2[:, 1]
        diff = cls.cpu().long() != want
        near = margin < MARGIN
        share_near = float(near.float().mean())
        share_diff = float(diff.float().mean())
        populated = int((torch.bincount(want.reshape(-1), minlength=classes) > 0).sum())
        print(f"[{name}/{head}] differing pixels {int(diff.sum())} ({100 * share_diff:.4f} %), oracle pixels under the margin "
              f"{100 * share_near:.4f} %, classes {torch.bincount(want.reshape(-1), minlength=classes).tolist()}")
        assert bool((~diff | near).all()), f"{int((diff & ~near).sum())} pixels differ with an oracle margin >= {MARGIN}"
        for i in range(b):
            assert float(diff[i].float().mean()) <= EXCUSED_CAP, (i, float(diff[i].float().mean()))
        assert populated >= 2
    assert o == eng.planes
    eng.close()


# ---- 6. the predictor paths ----
BASE_KEYS = {"sem_seg", "panoptic_seg", "eee_boundary"}


def _check_frame(out, masks_b, want_mask_hist=True):
    lg = out["eee_boundary"]
    cls = out["eee_boundary_classes"]
    assert cls.dtype == torch.uint8 and cls.shape == lg.shape[1:] and cls.is_cuda
    mine = torch.argmax(lg, dim=0)
    assert torch.equal(cls.long(), mine)
    assert torch.equal(out["eee_boundary_hist"].long(), torch.bincount(mine.reshape(-1), minlength=4))
    if want_mask_hist:
        mh = out["eee_boundary_mask_hist"]
        assert mh.shape == (len(masks_b), 4)
        assert np.array_equal(mh.cpu().numpy(), mask_hist_np(cls.cpu().numpy()[None], np.asarray(masks_b)[None], 4)[0])
        assert set(out) - {"instances"} == BASE_KEYS | {"eee_boundary_classes", "eee_boundary_hist", "eee_boundary_mask_hist"}
    else:
        assert set(out) - {"instances"} == BASE_KEYS | {"eee_boundary_classes", "eee_boundary_hist"}


def test_predictor_paths_with_and_without_decode_errors():
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
    h, w, n = 96, 128, 3
    batch, offs, image = _scene(3, 2, h, w, n)
    sd = loud_state_dict(1, image, offs, n)
    rgb, dep = batch["rgb"], batch["depth"]
    masks = [batch["masks"][0], batch["masks"][1][:2]]                       # 3 and 2 initial masks
    for tta in (False, True):
        pred = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, tta=tta, decode_errors=True)
        assert pred.decode_errors and pred.model.decode_errors
        _check_frame(pred.predict(rgb[0], dep[0], masks[0])[0], masks[0])                          # predict / predict_one
        _check_frame(pred.predict(rgb[1], dep[1], None)[0], np.zeros((0, h, w), np.uint8))         # no initial masks
        for o, m in zip(pred.predict_batch(rgb, dep, masks), masks):                               # predict_batch
            _check_frame(o, m)
        dm = dev(batch["masks"])
        hd = pred.model.enqueue_batch(dev(rgb), dev(dep), dm)                                      # enqueue / collect
        outs, ms = pred.model.collect_batch(hd)
        for o, m in zip(outs, batch["masks"]):
            _check_frame(o, m)
        if not tta:
            items = [{"image": image[i], "initial_pred_offset": torch.from_numpy(offs[i])} for i in range(2)]
            for o in pred.model(items):                                                            # model(list[dict]): no masks
                _check_frame(o, None, want_mask_hist=False)
        # off: exactly today's keys
        pred.model.decode_errors = False
        off = [pred.predict(rgb[0], dep[0], masks[0])[0]] + pred.predict_batch(rgb, dep, masks)
        off += pred.model.collect_batch(pred.model.enqueue_batch(dev(rgb), dev(dep), dm))[0]
        for o in off:
            assert set(o) - {"instances"} == BASE_KEYS
        pred.model.close()
    assert not MaskRefinerPredictor(None, device="cuda:0", state_dict=sd).model.decode_errors


# ---- 7. the adapter: scoring and visualisation ----
def test_adapter_score_and_visualize():
    from quber_amd.eval.refiner_model import MaskRefiner
    h, w, n = 96, 128, 3
    batch, offs, image = _scene(3, 1, h, w, n)
    sd = loud_state_dict(1, image, offs, n)
    for decode in (True, False):                     # the class map from the dict, or decoded from the logits on demand
        ref = MaskRefiner(None, weights_file=None, dataset="OSD", decode_errors=decode)
        ref.refiner_predictor.model.state_dict = sd
        out = ref.refiner_predictor.predict(batch["rgb"][0], batch["depth"][0], batch["masks"][0])[0]
        assert ("eee_boundary_classes" in out) == decode
        cls_np = torch.argmax(out["eee_boundary"], dim=0).cpu().numpy().astype(np.uint8)[None]
        init = (batch["masks"][0] != 0).astype(np.uint8)
        gt2 = (synth.make_scene(21, h, w, 4)["masks"] != 0).astype(np.uint8)
        for gt in (init, gt2):
            res = ref.score_error_maps(out, init, gt)
            assert list(res) == ["eee_boundary"]
            t = res["eee_boundary"]["confusion"]
            want = confusion_np(cls_np, errmaps_np.explicit_error_maps(init, gt)[None], 1, "e3")[0]
            assert np.array_equal(t, want) and int(t.sum()) == h * w
            if gt is init:
                assert int(t[2:].sum()) == 0 and int(t[0].sum()) > 0        # no FP / FN target by construction
            else:
                assert int(t[2].sum()) > 0 and int(t[3].sum()) > 0
            m = em.iou_from_confusion(want)
            for k in ("iou", "iou_all", "accuracy"):
                np.testing.assert_array_equal(res["eee_boundary"][k], m[k])
            np.testing.assert_array_equal(res["eee_boundary"]["iou_err"], em.iou_err(want, "e3"))
        vis = ref.visualize_errors(batch["rgb"][0], out)
        assert vis.dtype == np.uint8 and np.array_equal(vis, overlay_np(batch["rgb"], cls_np, em.DEFAULT_PALETTE["e3"])[0])
        assert not np.array_equal(vis, batch["rgb"][0])
        ref.refiner_predictor.model.close()


# ---- 8. hipGraph ----
def test_error_chain_graph_replay_equals_eager():
    """decode -> mask histogram -> score captured as one hipGraph (a straight chain) and replayed twice == the eager results, in a
    fresh child process (tests/error_graph_child.py), as tests/test_gpu_tta.py does for its step."""
    import json
    import os
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "error_graph_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["eager_equals_numpy"] and res["replay_equals_eager"] and res["second_replay_equals_eager"], res
    assert res["pixels"] > 0, res
