"""GPU: the connected-component clean-up of the refined instances (INTEGRATION.md "Connected-component clean-up"; csrc/cleanup.hip).

quber_cleanup_ids and quber_cleanup_postprocess against the numpy contract of tests/test_cleanup_cpu.py: ids, label maps, boxes and
reports exactly, scores within the project's bar (the foreground probabilities are summed with float64 atomic adds); the predictor with
``cleanup=`` against ``cleanup=None`` followed by the contract, and the iterative loop against the chain of single passes."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from oracle import encode_np
from quber_amd import engine, synth
from quber_amd.cleanup import Cleanup
from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
from test_cleanup_cpu import HAND, _structure, cleanup_np, cleanup_post_np, scenes

pytestmark = pytest.mark.gpu

SCORE_TOL = dict(rtol=2e-5, atol=1e-6)
SHAPES = [(70, 131), (33, 64)]
# (connectivity, keep_largest, min_island_area, max_hole_area): the two presets at areas that bite on small frames, islands, everything
# at once, nothing at all
OPTIONS = [(4, True, 0, 0), (8, False, 0, 40), (8, False, 12, 0), (4, False, 6, 9), (8, True, 0, 10 ** 6), (4, True, 0, 2), (8, False, 0, 0)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _engine(h, w, batch):
    return engine.Engine(engine.make_config(h, w, max_batch=batch, max_instances=1, with_network=False), "cuda:0")


_SCENES = {}


def _scenes(h, w):
    if (h, w) not in _SCENES:
        _SCENES[(h, w)] = scenes(h, w)
    return _SCENES[(h, w)]


def _run(eng, ids, n, o, shift=0):
    """quber_cleanup_ids on a copy of `ids` placed `shift` bytes into a guarded buffer -> (ids, report) on the host."""
    nbytes = ids.size * 4
    buf = torch.full((shift + nbytes + 64,), 0x3C, dtype=torch.uint8, device="cuda")
    d = buf[shift:shift + nbytes].view(torch.int32).view(ids.shape)
    d.copy_(dev(ids))
    out, rep = eng.cleanup_ids(d, n, Cleanup(o[1], o[0], o[2], o[3]))
    assert out.data_ptr() == d.data_ptr() and rep.shape == (ids.shape[0], n + 1, 4)
    assert bool((buf[:shift] == 0x3C).all()) and bool((buf[shift + nbytes:] == 0x3C).all())
    return d.cpu().numpy(), rep.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("h,w", SHAPES, ids=["70x131", "33x64"])
@pytest.mark.parametrize("name", ["row-and-frame-wrap", "serpentine", "checkerboard", "all-void", "all-one-instance", "n-ids-0", "id-254", "random",
                                  "random-fine", "hand-drawn-tiled"])
def test_cleanup_ids_equals_contract(h, w, name):
    ids, n = _scenes(h, w)[name]
    eng = _engine(h, w, ids.shape[0])
    for k, o in enumerate(OPTIONS):
        want, rep = cleanup_np(ids, n, *o)
        got, got_rep = _run(eng, ids, n, o, shift=4 * (k % 4))          # 4-byte-only alignments too
        np.testing.assert_array_equal(got, want, err_msg=f"{name} {o}")
        np.testing.assert_array_equal(got_rep, rep, err_msg=f"{name} {o}")
    eng.close()


@pytest.mark.parametrize("name", list(HAND))
def test_hand_drawn_threshold_and_tie_cases(name):
    """Equal-size components (the raster-first one wins), a hole of exactly a_h pixels (stays), an island of exactly a_i pixels
    (stays), a hole at the frame edge (filled), between two instances (stays), a speck of j inside i (becomes i) - at the drawings'
    own frame sizes, against the expectations written down by hand."""
    ids, n, o, want, rows = HAND[name]
    eng = _engine(ids.shape[1], ids.shape[2], 1)
    got, rep = _run(eng, ids, n, o)
    np.testing.assert_array_equal(got, want)
    for i, row in rows.items():
        assert tuple(rep[0, i]) == row, (i, rep[0])
    eng.close()


def test_second_call_overwrites_and_is_a_fixed_point():
    h, w = 70, 131
    ids, n = _scenes(h, w)["random"]
    eng = _engine(h, w, 3)
    for o in ((4, True, 0, 30), (8, False, 9, 12)):
        opts = Cleanup(o[1], o[0], o[2], o[3])
        want, rep = cleanup_np(ids, n, *o)
        d = dev(ids)
        report = torch.full((3, n + 1, 4), 77, dtype=torch.int32, device="cuda")
        eng.cleanup_ids(d, n, opts, report)
        np.testing.assert_array_equal(d.cpu().numpy(), want)
        np.testing.assert_array_equal(report.cpu().numpy(), rep)
        assert rep[:, 1:, 1].sum() > 0 and rep[:, 0, 2].sum() > 0
        eng.cleanup_ids(d, n, opts, report)                              # the same buffers again: what a graph replay does
        again, rep2 = cleanup_np(want, n, *o)
        np.testing.assert_array_equal(d.cpu().numpy(), want)
        np.testing.assert_array_equal(report.cpu().numpy(), rep2)
        assert not rep2[:, :, 1:3].any() and np.array_equal(again, want)
        # the report is optional in the C ABI
        d2 = dev(ids)
        engine._lib.check(eng.lib.quber_cleanup_ids(eng.h, engine._ptr(d2), 3, n, *opts.args(), None, engine._stream()))
        np.testing.assert_array_equal(d2.cpu().numpy(), want)
    # a batch below max_batch, and bad options
    d = dev(ids[:1])
    eng.cleanup_ids(d, n, "largest")
    np.testing.assert_array_equal(d.cpu().numpy(), cleanup_np(ids[:1], n, 4, True)[0])
    for bad in ((3, 6, 0, 0, 0), (3, 8, 2, 0, 0), (3, 8, 0, -1, 0), (3, 8, 0, 0, -1), (4, 8, 0, 0, 0)):
        assert eng.lib.quber_cleanup_ids(eng.h, engine._ptr(d), bad[0], n, *bad[1:], None, engine._stream()) != 0
    assert eng.lib.quber_cleanup_ids(eng.h, engine._ptr(d), 1, 255, 8, 0, 0, 0, None, engine._stream()) != 0
    eng.close()


# ---- quber_cleanup_postprocess on a realistic scene ----
def realistic_logits(h=480, w=640, b=2, n=8, noise=2.0):
    """Head outputs of `b` synth scenes with enough noise on the foreground logit and the offsets for specks (background pixels
    that turn foreground, votes for the wrong centre) and holes (foreground pixels that dip below zero)."""
    out = []
    for f in range(b):
        sc = synth.make_scene(500 + f, h, w, n)
        enc = encode_np.encode_initial_masks(sc["masks"])
        out.append(np.concatenate(synth.fake_head_outputs(enc, sc["masks"], np.random.default_rng(600 + f), noise=noise)))
    return np.stack(out).astype(np.float32)


def _host(post):
    return {k: v.cpu().numpy() for k, v in post.items()}


def test_cleanup_postprocess_realistic_scene():
    h, w, B = 480, 640, 2
    logits = realistic_logits(h, w, B)
    eng = _engine(h, w, B)
    d_logits = dev(logits)
    plain = _host(eng.postprocess(d_logits))
    assert plain["count"].min() >= 2
    # all options off: the label map and the boxes of plain post-processing, bit for bit; every component counted
    post = eng.postprocess(d_logits)
    rep = eng.cleanup_post(d_logits, post, Cleanup()).cpu().numpy()
    got = _host(post)
    for key in ("panoptic", "boxes", "labels", "count", "centers", "ncenters"):
        np.testing.assert_array_equal(got[key], plain[key], err_msg=key)
    np.testing.assert_allclose(got["scores"], plain["scores"], **SCORE_TOL)
    pan0, sc0, bx0, rep0 = cleanup_post_np(logits, plain["panoptic"], plain["labels"], plain["count"], Cleanup())
    np.testing.assert_array_equal(rep, rep0)
    np.testing.assert_array_equal(pan0, plain["panoptic"])
    assert not rep[:, :, 1:3].any() and (rep[:, 1:, 0] > 1).any()
    for opts in (Cleanup.uois(), Cleanup.sam(), Cleanup(False, 8, 50, 2)):
        post = eng.postprocess(d_logits)
        report = eng.cleanup_post(d_logits, post, opts)
        got = _host(post)
        pan, scores, boxes, rep = cleanup_post_np(logits, plain["panoptic"], plain["labels"], plain["count"], opts)
        np.testing.assert_array_equal(got["panoptic"], pan)
        np.testing.assert_array_equal(report.cpu().numpy(), rep)
        for b in range(B):
            k = int(plain["count"][b])
            np.testing.assert_array_equal(got["boxes"][b, :k], boxes[b, :k])
            np.testing.assert_allclose(got["scores"][b, :k], scores[b, :k], **SCORE_TOL)
            assert not got["boxes"][b, k:].any() and not got["scores"][b, k:].any()
            assert (rep[b, 1:k + 1, 3] > 0).all()                          # every instance keeps a pixel
        for key in ("labels", "count", "centers", "ncenters"):
            np.testing.assert_array_equal(got[key], plain[key], err_msg=key)
        assert rep[:, :, 1].sum() + rep[:, 0, 2].sum() > 0, "nothing to clean: the comparison is blind"
        assert not np.array_equal(pan, plain["panoptic"])
        # a second call on the same tables: overwritten report, nothing left to do
        again = eng.cleanup_post(d_logits, post, opts, report).cpu().numpy()
        np.testing.assert_array_equal(post["panoptic"].cpu().numpy(), pan)
        np.testing.assert_array_equal(post["boxes"].cpu().numpy(), got["boxes"])
        assert not again[:, :, 1:3].any() and np.array_equal(again[:, :, 3], rep[:, :, 3])
    eng.close()


# ---- end to end ----
def speck_logits(h=96, w=128, planes=8):
    """Logits built to yield a detached speck and a hole: two rectangular objects A (left) and B (right), each pixel's offset pointing
    at its object's centre; a 4 x 4 foreground patch beyond B whose offsets point at A's centre (it votes for A: a speck of A on the
    far side of B); a 3 x 3 dip of the foreground logit inside B.  The centre plane has one bump per object."""
    lg = np.zeros((1, planes, h, w), np.float32)
    lg[0, 0] = -4.0
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    for (y0, y1, x0, x1), (cy, cx) in ((((20, 70, 10, 50), (45, 30))), ((20, 70, 60, 100), (45, 80)), ((40, 44, 110, 114), (45, 30))):
        lg[0, 0, y0:y1, x0:x1] = 4.0
        lg[0, 2, y0:y1, x0:x1] = cy - yy[y0:y1, x0:x1]
        lg[0, 3, y0:y1, x0:x1] = cx - xx[y0:y1, x0:x1]
    for cy, cx in ((45, 30), (45, 80)):                      # a smooth bump per object: one local maximum, non-zero where the scores read it
        lg[0, 1] += 0.9 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 50.0)
    lg[0, 0, 40:43, 75:78] = -4.0
    return lg


def _predict_on(logits, **kw):
    """A predictor whose network output is `logits` whatever the frame: everything from post-processing on is the real path."""
    h, w = logits.shape[2:]
    sc = synth.make_scene(3, h, w, 2)
    pred = MaskRefinerPredictor(None, device="cuda:0", **kw)
    eng = pred.model.engine_for(h, w, 1, 2)
    assert eng.planes == logits.shape[1]
    d_logits = dev(logits)
    eng.forward = lambda bgr, depth, offsets, out=None: d_logits.clone()
    out = pred.predict(sc["rgb"], sc["depth"], sc["masks"])[0]
    res = {"panoptic": out["panoptic_seg"][0].cpu().numpy(), "keys": set(out)}
    if "instances" in out:
        inst = out["instances"]
        res.update(masks=inst.pred_masks.cpu().numpy(), boxes=inst.pred_boxes.tensor.cpu().numpy(), scores=inst.scores.cpu().numpy(),
                   fields=set(inst.get_fields()))
        for f in ("cc_components", "cc_removed", "cc_filled"):
            if inst.has(f):
                assert inst.get(f).dtype == torch.int64
                res[f] = inst.get(f).cpu().numpy()
    pred.model.close()
    return res


def _components(mask, c):
    return ndimage.label(mask, structure=_structure(c))[1]


def test_predictor_cleanup_equals_none_followed_by_the_contract():
    logits = speck_logits()
    none = _predict_on(logits)
    assert none["masks"].shape[0] == 2 and [_components(m, 4) for m in none["masks"]] == [2, 1], "the frame has no detached speck"
    assert "cc_removed" not in none and not ({"cc_components", "cc_removed", "cc_filled"} & none["fields"])
    labels = np.full((1, 200), -1, np.float32)
    labels[0, :2] = (1001, 1002)
    for opt, removed, filled in (("largest", [16, 0], [0, 0]), ("holes", [0, 0], [0, 9]), (Cleanup(True, 4, 0, 10), [16, 0], [0, 9])):
        got = _predict_on(logits, cleanup=opt)
        assert got["keys"] == none["keys"] and got["fields"] - none["fields"] == {"cc_components", "cc_removed", "cc_filled"}
        pan, scores, boxes, rep = cleanup_post_np(logits, none["panoptic"][None], labels, [2], Cleanup.parse(opt))
        np.testing.assert_array_equal(got["panoptic"], pan[0])
        np.testing.assert_array_equal(got["masks"], np.stack([pan[0] == 1001, pan[0] == 1002]))
        np.testing.assert_array_equal(got["boxes"], boxes[0, :2])
        np.testing.assert_allclose(got["scores"], scores[0, :2], **SCORE_TOL)
        assert got["cc_components"].tolist() == rep[0, 1:3, 0].tolist() == [2, 1]
        assert got["cc_removed"].tolist() == rep[0, 1:3, 1].tolist() == removed
        assert got["cc_filled"].tolist() == rep[0, 1:3, 2].tolist() == filled
        if Cleanup.parse(opt).keep_largest:
            assert [_components(m, 4) for m in got["masks"]] == [1, 1]
            assert got["boxes"][0].tolist() == [10, 20, 50, 70]


def test_iterations_with_cleanup_equal_the_chain_of_single_passes():
    from test_gpu_iterate import _case, _feedback, _k, _same_outputs
    h, w, n = 192, 256, 6
    batch, sd, _ = _case(h, w, 1, n)
    rgb, dep, masks = batch["rgb"][0], batch["depth"][0], batch["masks"][0]
    opts = Cleanup(True, 4, 0, 300)
    plain = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd)
    raw = plain.predict(rgb, dep, masks)[0]
    plain.model.close()
    one = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, cleanup=opts)
    first = one.predict(rgb, dep, masks)[0]
    assert _k(first) >= 1 and _k(first) == _k(raw)
    i1 = first["instances"]
    changed = int(i1.cc_removed.sum() + i1.cc_filled.sum())
    print(f"pass 1: {_k(first)} instances, components {i1.cc_components.tolist()}, removed {i1.cc_removed.tolist()}, filled {i1.cc_filled.tolist()}")
    assert changed > 0 and not torch.equal(first["panoptic_seg"][0], raw["panoptic_seg"][0]), "nothing to clean: the comparison is blind"
    assert all(_components(m, 4) == 1 for m in i1.pred_masks.cpu().numpy())
    want = one.predict(rgb, dep, _feedback(first, h, w))[0]
    # the batched and the streamed entry clean too
    hd = one.model.enqueue_batch(dev(rgb[None]), dev(dep[None]), dev(masks[None]))
    for o in (one.predict_batch(rgb[None], dep[None], [masks])[0], one.model.collect_batch(hd)[0][0]):
        assert _k(o) == _k(first) and o["instances"].cc_removed.dtype == torch.int64
        assert all(_components(m, 4) == 1 for m in o["instances"].pred_masks.cpu().numpy())
    one.model.close()
    two = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, iterations=2, cleanup=opts)
    got = two.predict(rgb, dep, masks)[0]
    two.model.close()
    assert got["refine_passes"] == 2 and _k(want) >= 1
    _same_outputs(got, want, "iterations=2, cleanup")
    for f in ("cc_components", "cc_removed", "cc_filled"):
        assert torch.equal(got["instances"].get(f), want["instances"].get(f)), f
    tta = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, tta=True, cleanup=opts)
    t = tta.predict(rgb, dep, masks)[0]
    tta.model.close()
    assert _k(t) >= 1 and all(_components(m, 4) == 1 for m in t["instances"].pred_masks.cpu().numpy())
