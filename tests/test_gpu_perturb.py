"""GPU: the perturbed initial masks (INTEGRATION.md "Perturbed initial masks"; csrc/perturb.hip).

quber_perturb_masks against the numpy contract of tests/test_perturb_cpu.py - masks and reports alike, exactly - with the bit planes in
LDS and in device memory; the clipping of malformed programs; the predictor with ``perturb=`` against ``perturb=None`` fed with the
contract's masks."""
import numpy as np
import pytest
import torch

from quber_amd import _lib, engine
from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
from quber_amd.perturb import Perturb
from test_perturb_cpu import ellipse, perturb_batch_np, perturb_np, scenes

pytestmark = pytest.mark.gpu

SHAPES = [(33, 64), (70, 131), (9, 20)]          # whole words; tail bits in the fifth word; less than one word
# (iou target, rounds): stops after 1-11 rounds; in round 1-3; never - all 24 operations run
CASES = [(0.8, 12), (0.95, 12), (0.0, 6)]
# rounds of the centred ellipse (mask [0, 0]) under seeds 0..5 at a target of 0.8
ROUNDS_08 = {(33, 64): [1, 2, 3, 5, 5, 3], (70, 131): [11, 6, 4, 5, 9, 9]}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _engine(h, w, batch):
    return engine.Engine(engine.make_config(h, w, max_batch=batch, max_instances=1, with_network=False), "cuda:0")


_WANT = {}


def _case(h, w, target, rounds, seed):
    """(masks, programs, targets, contract masks, contract report) of one case, computed once."""
    key = (h, w, target, rounds, seed)
    if key not in _WANT:
        masks = scenes(h, w)
        p = Perturb(target, seed=seed, rounds=rounds)
        progs, tg = p.programs(2, 3, h, w), p.targets(2, 3)
        _WANT[key] = (masks, progs, tg) + perturb_batch_np(masks, progs, tg)
    return _WANT[key]


def _guarded(shape, shift, fill=0x3C):
    n = int(np.prod(shape))
    buf = torch.full((shift + n + 64,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[shift:shift + n].view(shape)


def _run(eng, masks, progs, targets, placement, shift=1, out=None, report=None):
    """quber_perturb_masks with input and output `shift` / `shift + 2` bytes into guarded buffers -> (masks, report) on the host."""
    _, d_in = _guarded(masks.shape, shift + 2)
    d_in.copy_(dev(masks))
    buf, d_out = _guarded(masks.shape, shift) if out is None else out
    got, rep = eng.perturb_masks(d_in, dev(np.array(progs, np.int32)), dev(np.array(targets, np.float64)), d_out, report, placement)
    n = d_out.numel()
    assert got.data_ptr() == d_out.data_ptr() and rep.shape == masks.shape[:2] + (4,)
    assert bool((buf[:shift] == 0x3C).all()) and bool((buf[shift + n:] == 0x3C).all()), "wrote outside the output"
    np.testing.assert_array_equal(d_in.cpu().numpy(), masks, err_msg="the input changed")
    return d_out.cpu().numpy(), rep.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("placement", [1, 2], ids=["lds", "device-memory"])
@pytest.mark.parametrize("h,w", SHAPES, ids=["33x64", "70x131", "9x20"])
def test_perturb_equals_contract(h, w, placement):
    eng = _engine(h, w, 2)
    k = 0
    for target, rounds in CASES:
        for seed in range(6) if target == 0.8 else (0, 4):
            masks, progs, tg, want, rep = _case(h, w, target, rounds, seed)
            got, got_rep = _run(eng, masks, progs, tg, placement, shift=1 + 2 * (k % 3))
            k += 1
            print(f"{h}x{w} placement {placement} target {target} seed {seed}: rounds {rep[:, :, 0].ravel().tolist()}")
            np.testing.assert_array_equal(got_rep, rep, err_msg=f"target {target} seed {seed}")
            np.testing.assert_array_equal(got, want, err_msg=f"target {target} seed {seed}")
            assert set(np.unique(got)) <= {0, 255}
            assert not got[:, 1:].any()                                  # the empty mask and the one of values <= 127 stay empty
            assert (rep[:, 1, 0] == rounds).all()                        # empty against empty: iou = 1, never below the target
            assert (rep[:, 2, 0] == (1 if target > 0 else rounds)).all() # empty against a non-empty g: iou ~ 0, below any target > 0
            if target == 0.0:
                assert (rep[:, :, 0] == rounds).all()
            if target == 0.95 and (h, w) in ROUNDS_08:
                assert 1 <= rep[0, 0, 0] <= 3
            if target == 0.8 and (h, w) in ROUNDS_08:
                assert rep[0, 0, 0] == ROUNDS_08[(h, w)][seed]
            assert not np.array_equal(got[:, 0], (masks[:, 0] > 127) * 255), "nothing was perturbed: the comparison is blind"
    eng.close()


def test_frame_beyond_lds_runs_in_device_memory():
    h, w = 1024, 704                                                     # 3 x 90 KB of bit planes
    gt = (ellipse(h, w) * 255).astype(np.uint8)[None, None]
    p = Perturb(0.0, seed=1, rounds=3)
    progs, tg = p.programs(1, 1, h, w), p.targets(1, 1)
    want, rep = perturb_batch_np(gt, progs, tg)
    eng = _engine(h, w, 1)
    before = eng.workspace_bytes()
    got, got_rep = _run(eng, gt, progs, tg, 0)
    np.testing.assert_array_equal(got_rep, rep)
    np.testing.assert_array_equal(got, want)
    assert rep[0, 0, 0] == 3 and not np.array_equal(got, gt)
    assert eng.workspace_bytes() == before + 12 * h * 22                 # the workspace of one mask, allocated by this call
    with pytest.raises(_lib.QuberError, match="LDS"):
        _run(eng, gt, progs, tg, 1)
    got, got_rep = _run(eng, gt, progs, tg, 2)
    np.testing.assert_array_equal(got, want)
    assert eng.workspace_bytes() == before + 12 * h * 22                 # kept, not allocated again
    eng.close()


def test_second_call_overwrites_and_bad_arguments():
    h, w = 70, 131
    eng = _engine(h, w, 2)
    masks, progs, tg, want, rep = _case(h, w, 0.8, 12, 2)
    _, progs2, tg2, want2, rep2 = _case(h, w, 0.0, 6, 4)
    assert not np.array_equal(want, want2)
    for placement in (1, 2):
        out = _guarded(masks.shape, 3)
        report = torch.full((2, 3, 4), 77, dtype=torch.int32, device="cuda")
        got, got_rep = _run(eng, masks, progs, tg, placement, 3, out, report)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_rep, rep)
        got, got_rep = _run(eng, masks, progs2, tg2, placement, 3, out, report)       # the same buffers again: what a graph replay does
        np.testing.assert_array_equal(got, want2)
        np.testing.assert_array_equal(got_rep, rep2)
    # a batch below max_batch, per-mask targets, the report optional in the C ABI
    d_in, d_prog, d_out = dev(masks[:1]), dev(np.array(progs[:1])), torch.empty((1, 3, h, w), dtype=torch.uint8, device="cuda")
    mixed = np.array([[0.95, 0.5, 0.0]])
    call = lambda *a: eng.lib.quber_perturb_masks(eng.h, *a, engine._stream())
    P = engine._ptr
    assert call(P(d_in), 1, 3, P(d_prog), 48, 4, P(dev(mixed)), P(d_out), None, 0) == 0
    np.testing.assert_array_equal(d_out.cpu().numpy(), perturb_batch_np(masks[:1], progs[:1], mixed)[0])
    d_tg = dev(tg[:1])
    assert call(P(d_in), 1, 3, P(d_prog), 48, 4, P(d_tg), P(d_in), None, 0) != 0 and b"overlap" in eng.lib.quber_last_error()
    assert call(P(d_in), 1, 3, P(d_prog), 48, 4, P(d_tg), P(d_in.view(-1)[h * w:]), None, 0) != 0          # partly overlapping
    assert call(P(d_in), 1, 3, P(d_prog), 48, 4, P(d_tg), P(d_out), None, 3) != 0                            # no such placement
    assert call(P(d_in), 1, 3, P(d_prog), 46, 4, P(d_tg), P(d_out), None, 0) != 0                            # half a round
    assert call(P(d_in), 1, 3, P(d_prog), 48, 0, P(d_tg), P(d_out), None, 0) != 0
    assert call(P(d_in), 3, 3, P(d_prog), 48, 4, P(d_tg), P(d_out), None, 0) != 0                            # above max_batch
    assert call(P(d_in), 1, 3, P(d_prog), 48, 4, None, P(d_out), None, 0) != 0
    np.testing.assert_array_equal(d_in.cpu().numpy(), masks[:1])
    eng.close()


@pytest.mark.parametrize("h,w", [(9, 20), (70, 131)], ids=["9x20", "70x131"])
def test_malformed_program_is_clipped(h, w):
    """Rectangles beyond the frame, negative corners, empty rectangles with the cleared pixel inside and outside the frame, sizes of 40, 0
    and -4, choices that do not exist: the kernel clips as the contract does, writes nothing outside the masks and returns normally."""
    masks = scenes(h, w)
    rng = np.random.RandomState(5)
    progs = np.empty((2, 3, 8, 8), np.int32)
    progs[..., 0] = rng.randint(-w, 2 * w, progs.shape[:3])
    progs[..., 1] = rng.randint(-h, 2 * h, progs.shape[:3])
    progs[..., 2] = rng.randint(-w, 3 * w, progs.shape[:3])
    progs[..., 3] = rng.randint(-h, 3 * h, progs.shape[:3])
    progs[..., 4:6] = rng.randint(0, 2, progs.shape[:3] + (2,))
    progs[..., 6] = rng.choice([40, 0, -4, 15, 16, 2 ** 31 - 1, 7], progs.shape[:3])
    progs[..., 7] = rng.choice([0, 1, 2, 3, 4, 5, -1], progs.shape[:3])
    progs[:, :, 0] = (-5, -3, 40 * w, 40 * h, 1, 1, 40, 2)                        # the whole frame and more, size 40
    progs[:, :, 1] = (w // 2 + 2, h // 2, w // 2 - 3, h // 2, 1, 0, 3, 1)        # empty; its cleared pixel lies inside the frame
    progs[:, :, 2] = (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0, 3, 2)
    tg = np.zeros((2, 3))
    want, rep = perturb_batch_np(masks, progs, tg)
    assert (rep[:, :, 0] == 2).all() and want[:, 0].any()
    eng = _engine(h, w, 2)
    for placement in (1, 2):
        got, got_rep = _run(eng, masks, progs, tg, placement, shift=1)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_rep, rep)
    eng.close()


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


def test_predictor_perturb_equals_none_fed_with_the_contract():
    from quber_amd import synth
    from test_gpu_cleanup import speck_logits
    h, w, n = 96, 128, 3
    logits = speck_logits(h, w)
    sc = [synth.make_scene(3 + b, h, w, 2) for b in range(2)]
    rgb, dep = np.stack([s["rgb"] for s in sc]), np.stack([s["depth"] for s in sc])
    masks = np.zeros((2, n, h, w), np.uint8)
    for b in range(2):
        masks[b, 0] = ellipse(h, w, h * (0.4 + 0.1 * b), w * 0.5) * 255
        masks[b, 1] = ellipse(h, w, h * 0.5, w * (0.3 + 0.3 * b), h / 5, w / 6) * 255
        masks[b, 2] = ellipse(h, w, h * 0.6, w * 0.6, h / 4, w / 8) * (200 if b else 100)        # frame 0: g without seg
    opts = Perturb(0.8, seed=3)

    def contract(frames, rows):
        """The contract on the frames a call uploads: mask i of frame b walks the program of seed 3 + b * rows + i."""
        m = masks[:frames, :rows]
        return perturb_batch_np(m, opts.programs(frames, rows, h, w), opts.targets(frames, rows))

    want1, rep1 = contract(1, n)
    want2, rep2 = contract(2, n)
    assert 1 <= rep1[0, 0, 0] < 250 and 1 <= rep1[0, 1, 0] < 250 and rep1[0, 2].tolist()[:2] == [1, 0]
    assert not np.array_equal(want1[0, :2], masks[0, :2])

    def same(a, b, what):
        assert set(a) - {"perturbed_masks", "perturb_report"} == set(b), what
        assert torch.equal(a["panoptic_seg"][0], b["panoptic_seg"][0]) and torch.equal(a["sem_seg"], b["sem_seg"]), what
        for key in ("initial_overlap",):
            if key in b:
                assert torch.equal(a[key], b[key]), (what, key)

    for kw in (dict(), dict(tta=True, iterations=2, track_initial=True)):
        got_off, want_off = [], []
        pert = _predictor(h, w, logits, got_off, perturb=opts, **kw)
        none = _predictor(h, w, logits, want_off, **kw)
        # predict(): one frame
        a = pert.predict(rgb[0], dep[0], masks[0])[0]
        b = none.predict(rgb[0], dep[0], want1[0])[0]
        assert "perturbed_masks" not in b and "perturb_report" not in b
        np.testing.assert_array_equal(a["perturbed_masks"].cpu().numpy(), want1[0])
        assert a["perturb_report"].dtype == torch.int64
        np.testing.assert_array_equal(a["perturb_report"].cpu().numpy(), rep1[0])
        same(a, b, "predict")
        # a bool mask counts as 0 / 255
        a = pert.predict(rgb[0], dep[0], masks[0] > 127)[0]
        np.testing.assert_array_equal(a["perturbed_masks"].cpu().numpy()[:2], want1[0, :2])
        none.predict(rgb[0], dep[0], want1[0])                               # (keeps the two records of forwards aligned)
        # predict_batch(): two frames, the second with one mask less (its padded row stays empty and runs no morphology)
        lists = [masks[0], masks[1, :2]]
        padded = masks.copy()
        padded[1, 2] = 0
        wantb, repb = perturb_batch_np(padded[:, :2], opts.programs(2, n, h, w)[:, :2], opts.targets(2, 2))
        outs = pert.predict_batch(rgb, dep, lists)
        refs = none.predict_batch(rgb, dep, [np.concatenate([wantb[0], want2[0, 2:]]), wantb[1]])
        for f, (a, b) in enumerate(zip(outs, refs)):
            k = len(lists[f])
            assert a["perturbed_masks"].shape == (k, h, w) and a["perturb_report"].shape == (k, 4)
            np.testing.assert_array_equal(a["perturbed_masks"].cpu().numpy()[:2], wantb[f])
            np.testing.assert_array_equal(a["perturb_report"].cpu().numpy()[:2], repb[f])
            same(a, b, "predict_batch")
        np.testing.assert_array_equal(outs[0]["perturbed_masks"].cpu().numpy()[2], want2[0, 2])
        if not kw:
            # the batched stream's entry
            hd = pert.model.enqueue_batch(dev(rgb), dev(dep), dev(masks))
            hr = none.model.enqueue_batch(dev(rgb), dev(dep), dev(want2))
            for f, (a, b) in enumerate(zip(pert.model.collect_batch(hd)[0], none.model.collect_batch(hr)[0])):
                np.testing.assert_array_equal(a["perturbed_masks"].cpu().numpy(), want2[f])
                np.testing.assert_array_equal(a["perturb_report"].cpu().numpy(), rep2[f])
                same(a, b, "enqueue_batch")
        # what the network was given - the encoding of the perturbed masks, of their mirrors under tta, of the fed-back instances in
        # pass 2 - is the same in both predictors, bit for bit
        assert len(got_off) == len(want_off) >= 3
        for x, y in zip(got_off, want_off):
            assert x.shape == y.shape and torch.equal(x, y)
        pert.model.close()
        none.model.close()
    with pytest.raises(ValueError):
        MaskRefinerPredictor(None, device="cuda:0", perturb=0.8)
