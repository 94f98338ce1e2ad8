"""GPU: the mask NMS on the device (csrc/masknms.hip through Engine.mask_nms and MaskRefinerPredictor(nms=...)) against its numpy
contract (tests/test_masknms_cpu.py: mask_nms_np).  Integers, bits and one float32 expression: every comparison is exact."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from quber_amd import engine
from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
from quber_amd.masknms import MaskNMS
from quber_amd.perturb import Perturb
from test_masknms_cpu import hand_cases, mask_nms_batch_np, mask_nms_np, proposals

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(ROOT, "quber_amd", "csrc", "masknms.hip")).read()
TILE = int(re.search(r"constexpr int MN_TILE = (\d+);", _SRC).group(1))        # masks per side of a gram tile
CHUNK = int(re.search(r"constexpr int MN_CHUNK = (\d+);", _SRC).group(1))      # words of a bit plane per gram block
# less than one word per row; whole words (16-byte aligned rows); tail bits, and 70 * 5 = 350 words: neither a multiple of the 256 words
# a pack block takes nor of the 4 words a plane is padded to; CHUNK + 1 words: the second gram chunk holds one word (and its padding)
SHAPES = [(9, 20), (33, 64), (70, 131), (41, 32 * (CHUNK + 1) // 41)]
COUNTS = [1, TILE - 1, TILE, TILE + 1, 40]
CAP = 64
FILL = 0x3C


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_ENGINES = {}


def _engine(h, w, batch=3, cap=CAP):
    key = (h, w, batch, cap)
    if key not in _ENGINES:
        _ENGINES[key] = engine.Engine(engine.make_config(h, w, max_batch=batch, max_instances=cap, with_network=False), "cuda:0")
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    torch.cuda.synchronize()
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


class Guarded:
    """The five outputs of a call, each `shift` elements into a buffer filled with a sentinel byte."""

    def __init__(self, B, N, h, w, shift):
        self.shift, self.bufs, self.views = shift, {}, {}
        for name, shape, dtype in (("out", (B, N, h, w), torch.uint8), ("ids", (B, h, w), torch.int32), ("source", (B, N), torch.int32),
                                   ("out_scores", (B, N), torch.float32), ("report", (B, 4), torch.int32)):
            n = int(np.prod(shape))
            raw = torch.full(((shift + n + 64) * torch.empty((), dtype=dtype).element_size(),), FILL, dtype=torch.uint8, device="cuda")
            buf = raw.view(dtype)
            self.bufs[name], self.views[name] = (raw, n), buf[shift:shift + n].view(shape)

    def intact(self):
        for name, (raw, n) in self.bufs.items():
            es = raw.numel() // (self.shift + n + 64)
            if not (bool((raw[:self.shift * es] == FILL).all()) and bool((raw[(self.shift + n) * es:] == FILL).all())):
                return False
        return True


def _run(eng, masks, scores, nms, shift=16, guarded=None):
    """Engine.mask_nms into guarded outputs, the input `shift` bytes into its allocation -> the five results on the host."""
    B, N, h, w = masks.shape
    d_in = torch.full((shift + masks.size + 64,), FILL, dtype=torch.uint8, device="cuda")[shift:shift + masks.size].view(masks.shape)
    d_in.copy_(dev(masks))
    g = Guarded(B, N, h, w, shift) if guarded is None else guarded
    v = g.views
    r = eng.mask_nms(d_in, dev(np.asarray(scores, np.float32)), nms, v["out"], v["ids"], v["source"], v["out_scores"], v["report"])
    assert r["masks"].data_ptr() == v["out"].data_ptr()
    torch.cuda.synchronize()
    assert g.intact(), "wrote outside an output"
    np.testing.assert_array_equal(d_in.cpu().numpy(), masks, err_msg="the input changed")
    return tuple(v[k].cpu().numpy() for k in ("out", "ids", "source", "out_scores", "report"))


def _same(got, want, what=""):
    for name, a, b in zip(("masks", "ids", "source", "scores", "report"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b,
                                      err_msg="%s %s" % (what, name))


_SETS = {}


def _sets(h, w, n):
    """Two frames of n proposals (one with distinct scores and areas, one full of ties), and the contract on them for both on_top."""
    key = (h, w, n)
    if key not in _SETS:
        a, b = proposals(h, w, n, 100 + n), proposals(h, w, n, 200 + n, distinct=False, value=1)
        masks, scores = np.stack([a[0], b[0]]), np.stack([a[1], b[1]])
        _SETS[key] = (masks, scores, {t: mask_nms_batch_np(masks, scores, 0.7, t) for t in ("large", "small")})
    return _SETS[key]


def test_shapes_are_what_they_claim():
    h, w = SHAPES[3]
    assert h * ((w + 31) // 32) == CHUNK + 1 and w % 16 == 0
    assert (70 * 5) % 256 and (70 * 5) % 4 and TILE >= 2 and COUNTS[-1] > 2 * TILE


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("h,w", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_mask_nms_equals_contract(h, w, n):
    masks, scores, want = _sets(h, w, n)
    eng = _engine(h, w)
    # 16 bytes into the allocations (the 16-byte paths where the shape allows them) and 1 element in (the byte paths)
    for on_top, shift in (("large", 16), ("small", 16), ("large", 1), ("small", 3)):
        got = _run(eng, masks, scores, MaskNMS(0.7, on_top), shift)
        _same(got, want[on_top], "%dx%d n=%d %s shift %d" % (h, w, n, on_top, shift))
    assert want["large"][4][:, 0].max() >= 1


def test_three_frames_with_different_counts_and_a_padded_frame():
    h, w, n = 70, 131, 12
    sets = [proposals(h, w, n, 300 + b, distinct=bool(b % 2)) for b in range(3)]
    masks, scores = np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])
    scores[2, 8:] = np.nan                                   # frame 2 has 8 masks: the rest is not there
    want = mask_nms_batch_np(masks, scores)
    assert len(set(want[4][:, 0].tolist())) == 3, want[4]
    alone = mask_nms_np(masks[2, :8], scores[2, :8])
    np.testing.assert_array_equal(want[0][2, :8], alone[0])
    assert want[4][2].tolist() == [alone[1], alone[3], 0, 0]
    eng = _engine(h, w)
    _same(_run(eng, masks, scores, MaskNMS()), want)
    _same(_run(eng, masks, scores, None, shift=1), want)    # the default options are the reference's


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_built_cases_on_the_device(name):
    masks, scores, want = hand_cases()[name]
    eng = _engine(9, 20)
    for on_top, (count, kept, source) in want.items():
        got = _run(eng, masks[None], scores[None], MaskNMS(0.7, on_top), shift=1)
        _same(got, mask_nms_batch_np(masks[None], scores[None], 0.7, on_top), name + " " + on_top)
        assert got[4][0].tolist() == [count, kept, 0, 0] and got[2][0, :count].tolist() == source


def test_threshold_is_an_argument():
    h, w, n = 33, 64, 17
    masks, scores, _ = _sets(h, w, n)
    eng = _engine(h, w)
    seen = set()
    for thresh in (0.0, 0.3, 1.0):
        want = mask_nms_batch_np(masks, scores, thresh)
        _same(_run(eng, masks, scores, MaskNMS(thresh)), want, "thresh %g" % thresh)
        seen.add(tuple(want[4][:, 1].tolist()))
    assert len(seen) == 3


def test_second_call_overwrites_and_in_place():
    h, w = 70, 131
    eng = _engine(h, w)
    m1, s1, w1 = _sets(h, w, 17)
    m2, s2 = np.ascontiguousarray(m1[:, ::-1][:, :17]), np.ascontiguousarray(s1[::-1, ::-1])
    m2[0, 3:] = 0                                            # far fewer visible masks than the first call left behind
    want2 = mask_nms_batch_np(m2, s2, 0.7, "small")
    assert want2[4][0, 0] < w1["large"][4][0, 0] and not np.array_equal(want2[0], w1["large"][0])
    g = Guarded(2, 17, h, w, 16)
    _same(_run(eng, m1, s1, MaskNMS(), 16, g), w1["large"])
    _same(_run(eng, m2, s2, MaskNMS(on_top="small"), 16, g), want2, "second call")     # the same buffers again: what a graph replay does
    # the output may be the input itself
    d = dev(m1)
    r = eng.mask_nms(d, dev(s1), MaskNMS(), out=d)
    np.testing.assert_array_equal(d.cpu().numpy(), w1["large"][0])
    np.testing.assert_array_equal(r["report"].cpu().numpy(), w1["large"][4])
    # no masks at all: the id map and the report are cleared
    ids, rep = torch.full((2, h, w), 7, dtype=torch.int32, device="cuda"), torch.full((2, 4), 7, dtype=torch.int32, device="cuda")
    empty = torch.empty((2, 0, h, w), dtype=torch.uint8, device="cuda")
    eng.mask_nms(empty, torch.empty((2, 0), dtype=torch.float32, device="cuda"), ids=ids, report=rep)
    assert not bool(ids.any()) and not bool(rep.any())


def test_bad_arguments_are_refused_and_launch_nothing():
    h, w, n = 33, 64, 4
    eng = _engine(h, w)
    masks, scores = proposals(h, w, n, 7)
    d_m, d_s = dev(masks[None]), dev(scores[None])
    g = Guarded(1, CAP + 1, h, w, 4)
    v = g.views
    P = engine._ptr
    call = lambda e, *a: e.lib.quber_mask_nms(e.h, *a, engine._stream())
    outs = (P(v["out"]), P(v["ids"]), P(v["source"]), P(v["out_scores"]), P(v["report"]))
    before = eng.lib.quber_workspace_bytes(eng.h)
    assert call(eng, P(d_m), P(d_s), 1, CAP + 1, 0.7, 0, *outs) != 0 and b"n_masks" in eng.lib.quber_last_error()    # above max_instances
    assert call(eng, P(d_m), P(d_s), 1, -1, 0.7, 0, *outs) != 0
    assert call(eng, P(d_m), P(d_s), 4, n, 0.7, 0, *outs) != 0                                                       # above max_batch
    assert call(eng, P(d_m), P(d_s), 1, n, 0.7, 2, *outs) != 0                                                       # no such on_top
    assert call(eng, P(d_m), P(d_s), 1, n, float("nan"), 0, *outs) != 0
    assert call(eng, None, P(d_s), 1, n, 0.7, 0, *outs) != 0 and b"null" in eng.lib.quber_last_error()
    assert call(eng, P(d_m), None, 1, n, 0.7, 0, *outs) != 0
    for k in range(5):
        assert call(eng, P(d_m), P(d_s), 1, n, 0.7, 0, *[None if j == k else o for j, o in enumerate(outs)]) != 0
    assert call(eng, P(d_m), P(d_s), 1, n, 0.7, 0, P(d_m.view(-1)[h * w:]), *outs[1:]) != 0 and b"overlap" in eng.lib.quber_last_error()
    # a frame of more than 2^24 pixels: refused before any pointer is looked at (a context without a network at that size is a few
    # hundred MB of workspaces, no launch)
    big = _engine(4097, 4096, 1, 1)
    assert call(big, P(d_m), P(d_s), 1, 1, 0.7, 0, *outs) != 0 and b"2^24" in big.lib.quber_last_error()
    # more masks than the kernels' own limit, whatever max_instances says
    wide = _engine(9, 20, 1, 2048)
    assert call(wide, P(d_m), P(d_s), 1, 1025, 0.7, 0, *outs) != 0 and b"1024" in wide.lib.quber_last_error()
    torch.cuda.synchronize()
    assert g.intact() and all(bool((x.view(torch.uint8) == FILL).all()) for x in v.values()), "a refused call wrote"
    assert eng.lib.quber_workspace_bytes(eng.h) == before, "a refused call allocated"
    # the first good call allocates the workspace, which quber_workspace_bytes then counts; later calls allocate nothing
    fresh = _engine(h, w, 1, 8)
    b0 = fresh.lib.quber_workspace_bytes(fresh.h)
    fresh.mask_nms(d_m, d_s)
    b1 = fresh.lib.quber_workspace_bytes(fresh.h)
    fresh.mask_nms(d_m, d_s)
    assert b1 > b0 and fresh.lib.quber_workspace_bytes(fresh.h) == b1


# ---- end to end ----
def _predictor(h, w, logits, sink, **kw):
    """A predictor whose network output is `logits` whatever the frame and which records the encoded initial masks it was given:
    everything before and after the network is the real path."""
    pred = MaskRefinerPredictor(None, device="cuda:0", **kw)
    eng = pred.model.engine_for(h, w, 4, 64)
    d_logits = dev(logits)

    def forward(bgr, depth, offsets, out=None):
        sink.append(offsets.clone())
        return d_logits.expand(bgr.shape[0], -1, -1, -1).clone()
    eng.forward = forward
    return pred


def _equal(a, b, path):
    """Bit for bit, through tensors, tuples and Instances."""
    if isinstance(b, torch.Tensor):
        assert isinstance(a, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
    elif isinstance(b, (tuple, list)):
        assert len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, "%s[%d]" % (path, k))
    elif hasattr(b, "get_fields"):
        fa, fb = a.get_fields(), b.get_fields()
        assert set(fa) == set(fb), path
        for k in fb:
            _equal(fa[k].tensor if hasattr(fa[k], "tensor") else fa[k], fb[k].tensor if hasattr(fb[k], "tensor") else fb[k], path + "." + k)
    else:
        assert a == b, path


NMS_KEYS = {"nms_masks", "nms_source", "nms_scores", "nms_report"}


@pytest.mark.parametrize("variant", ["plain", "perturb"])
def test_predictor_nms_equals_none_fed_with_the_contract(variant):
    """MaskRefinerPredictor(nms=MaskNMS()) on overlapping proposals = the same predictor without nms fed the contract's masks, in every
    output key; with perturb= set as well, the perturbation acts on the NMS's output (one walk for all masks - a seed that broadcasts -
    because the two predictors run it on different numbers of planes)."""
    from quber_amd import synth
    from test_gpu_cleanup import speck_logits
    h, w = 96, 128
    logits = speck_logits(h, w)
    sc = [synth.make_scene(3 + b, h, w, 2) for b in range(2)]
    rgb, dep = np.stack([s["rgb"] for s in sc]), np.stack([s["depth"] for s in sc])
    sets = [proposals(h, w, 9, 41), proposals(h, w, 6, 42, distinct=False)]        # the second frame has fewer proposals, and ties
    lists, scores = [s[0] for s in sets], [s[1] for s in sets]
    want = [mask_nms_np(m, s) for m, s in zip(lists, scores)]
    assert all(1 <= r[1] < len(m) for r, m in zip(want, lists)) and want[0][1] != want[1][1]
    fed = [r[0][:r[1]] for r in want]
    if variant == "plain":
        kw = dict(decode_errors=True, track_initial=True, tta=True, iterations=2)
    else:
        kw = dict(decode_errors=True, perturb=Perturb(0.8, seeds=np.array([[3]]), rounds=20))
    got_off, want_off = [], []
    with_nms = _predictor(h, w, logits, got_off, nms=MaskNMS(), **kw)
    none = _predictor(h, w, logits, want_off, **kw)

    def check(a, b, f, what):
        assert set(a) - NMS_KEYS == set(b) and NMS_KEYS <= set(a) and not NMS_KEYS & set(b), (what, sorted(a), sorted(b))
        for key in b:
            _equal(a[key], b[key], "%s frame %d: %s" % (what, f, key))
        r = want[f]
        np.testing.assert_array_equal(a["nms_masks"].cpu().numpy(), r[0][:r[1]])
        assert a["nms_source"].dtype == torch.int64 and a["nms_report"].dtype == torch.int64
        np.testing.assert_array_equal(a["nms_source"].cpu().numpy(), r[2][:r[1]])
        np.testing.assert_array_equal(a["nms_scores"].cpu().numpy(), r[5][:r[1]])
        assert a["nms_report"].tolist() == [r[1], r[3]]

    outs = with_nms.predict_batch(rgb, dep, lists, scores)
    refs = none.predict_batch(rgb, dep, fed)
    for f, (a, b) in enumerate(zip(outs, refs)):
        check(a, b, f, "predict_batch")
    if variant == "perturb":
        assert not np.array_equal(outs[0]["perturbed_masks"].cpu().numpy(), fed[0])          # the walk did something - to the NMS's output
        # predict(): one frame, bool masks
        a = with_nms.predict(rgb[1], dep[1], lists[1] != 0, scores[1])[0]
        b = none.predict_batch(rgb[1:], dep[1:], fed[1:])[0]
        check(a, b, 1, "predict")
        # the batched stream's entry: device tensors, NaN scores where a frame has fewer masks
        n = max(len(m) for m in lists)
        dm, ds = np.zeros((2, n, h, w), np.uint8), np.full((2, n), np.nan, np.float32)
        for f in range(2):
            dm[f, :len(lists[f])], ds[f, :len(lists[f])] = lists[f], scores[f]
        nf = max(len(m) for m in fed)
        df = np.zeros((2, nf, h, w), np.uint8)
        for f in range(2):
            df[f, :len(fed[f])] = fed[f]
        hd = with_nms.model.enqueue_batch(dev(rgb), dev(dep), dev(dm), d_scores=dev(ds))
        hr = none.model.enqueue_batch(dev(rgb), dev(dep), dev(df), n_masks=[len(m) for m in fed])
        for f, (a, b) in enumerate(zip(with_nms.model.collect_batch(hd)[0], none.model.collect_batch(hr)[0])):
            for key in ("perturbed_masks", "perturb_report"):                    # (the stream keeps all rows of the mask histograms)
                _equal(a[key], b[key], "enqueue_batch frame %d: %s" % (f, key))
            _equal(a["panoptic_seg"], b["panoptic_seg"], "enqueue_batch panoptic")
            np.testing.assert_array_equal(a["nms_masks"].cpu().numpy(), fed[f])
    # what the network was given - the encoding of the NMS's masks, of their mirrors under tta, of the fed-back instances in pass 2 - is
    # the same in both predictors, bit for bit
    assert len(got_off) == len(want_off) >= 2
    for x, y in zip(got_off, want_off):
        assert x.shape == y.shape and torch.equal(x, y)
    with pytest.raises(ValueError):
        with_nms.predict_batch(rgb, dep, lists)
    with_nms.model.close()
    none.model.close()


def test_adapter_predict_and_stream_with_nms(tmp_path):
    """MaskRefiner(nms=MaskNMS()) on files: predict(..., mask_scores=) and predict_stream(batch=2) with the scores as the items' fifth
    element.  What the NMS hands to the refiner does not depend on the network and equals the contract exactly on both routes; the
    refined output of a frame run alone and in a batch of two agrees within the suite's batch-invariance bars (1e-4 on sem_seg, 0.9999
    of the label-map pixels: profiles/r20_batch_invariance.txt)."""
    from PIL import Image
    from quber_amd import synth
    from quber_amd.eval.refiner_model import MaskRefiner
    h, w = 480, 640
    items, want = [], []
    for i, n in enumerate((7, 5, 7)):
        sc = synth.make_scene(70 + i, h, w, 2)
        masks, scores = proposals(h, w, n, 500 + i, distinct=bool(i % 2))
        Image.fromarray(sc["rgb"][:, :, ::-1].copy()).save(tmp_path / f"rgb{i}.png")
        Image.fromarray(sc["depth"][:, :, 0].astype(np.uint16) * 5 + 300).save(tmp_path / f"depth{i}.png")
        items.append((str(tmp_path / f"rgb{i}.png"), str(tmp_path / f"depth{i}.png"), masks != 0, None, scores))
        want.append(mask_nms_np(masks, scores))
    assert all(1 <= r[1] < len(it[2]) for r, it in zip(want, items))
    ref = MaskRefiner(None, weights_file=None, dataset="OSD", nms=MaskNMS())
    assert ref.refiner_predictor.nms == MaskNMS() and ref.refiner_predictor.model.nms == MaskNMS()
    with pytest.raises(ValueError, match="required"):
        ref.predict(*items[0][:3])
    with pytest.raises(ValueError, match="finite"):
        ref.predict(*items[0][:3], mask_scores=np.full((7,), np.inf))
    seq = [ref.predict(*it[:4], mask_scores=it[4]) for it in items]
    got = list(ref.predict_stream(items, workers=2, batch=2))                # 2 + 1 frames; frame 1 has fewer proposals than frame 0
    assert len(got) == 3
    for i, ((m0, o0, _, _), (m1, o1, _, _)) in enumerate(zip(seq, got)):
        r = want[i]
        for o in (o0, o1):
            np.testing.assert_array_equal(o["nms_masks"].cpu().numpy(), r[0][:r[1]])
            np.testing.assert_array_equal(o["nms_source"].cpu().numpy(), r[2][:r[1]])
            np.testing.assert_array_equal(o["nms_scores"].cpu().numpy(), r[5][:r[1]])
            assert o["nms_report"].tolist() == [r[1], r[3]]
        d = float((o0["sem_seg"] - o1["sem_seg"]).abs().max())
        eq = float((o0["panoptic_seg"][0] == o1["panoptic_seg"][0]).float().mean())
        print(f"adapter nms frame {i}: max |sem_seg batch 1 - batch 2| = {d:.3e}, equal label-map pixels = {eq:.6f}")
        assert d < 1e-4 and eq > 0.9999 and len(m0) == len(m1)
    ref.refiner_predictor.model.close()
