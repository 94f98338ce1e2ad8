"""GPU: the validation losses on the device (csrc/losses.hip through Engine.loss_targets / Engine.losses and the predictor's losses= option)
against their contract (tests/test_losses_cpu.py).  The targets are compared bit for bit.  The loss values are sums of non-negative float64
terms of float32 inputs: against the float64 contract on the SAME inputs the relative error is at most N * 2^-53 (N <= 2^22 summed terms at
these sizes: 5e-10) plus a few ulp of exp / log1p - the bar is 1e-9 relative, 1e-300 absolute for exact zeros; it is derived, not measured.
The k-th value and the count above it are selections and must match exactly."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from quber_amd import _lib, engine
from quber_amd import losses as ls
from quber_amd.losses import Losses
from test_losses_cpu import blob_labels, golden_cases, load_case, loss_inputs, loss_targets_np, losses_ref, spec, target_planes

pytestmark = pytest.mark.gpu

REL, ABS = 1e-9, 1e-300
FILL = 0x3C
_ES = {torch.uint8: 1, torch.int32: 4, torch.float32: 4, torch.float64: 8}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_ENGINES = {}


def _engine(h, w, batch=3, legacy=0, tag=""):
    key = (h, w, batch, legacy, tag)
    if key not in _ENGINES:
        qc = engine.make_config(h, w, max_batch=batch, max_instances=64, with_network=False)
        qc.encode_legacy_f32 = legacy
        _ENGINES[key] = engine.Engine(qc, "cuda:0")
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    torch.cuda.synchronize()
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


class Arena:
    """Device tensors inside allocations filled with a sentinel byte, `shift` elements past an aligned address (0: aligned; 1: not 16-byte
    aligned, so the kernels take their lane-per-element form)."""

    def __init__(self, shift):
        self.shift, self.raw = shift, []

    def empty(self, shape, dtype):
        es = _ES[dtype]
        off, n = 64 + self.shift * es, int(np.prod(shape)) * es
        raw = torch.full((off + n + 64,), FILL, dtype=torch.uint8, device="cuda")
        self.raw.append((raw, off, n))
        return raw[off:off + n].view(dtype).view(tuple(shape))

    def intact(self):
        return all(bool((raw[:off] == FILL).all()) and bool((raw[off + n:] == FILL).all()) for raw, off, n in self.raw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _want_targets(labels, n, sp, legacy=False):
    ts = [loss_targets_np(lab, n, sp.sigma, sp.small_area, sp.small_weight, legacy_f32=legacy) for lab in labels]
    return (np.stack([target_planes(t) for t in ts]), np.stack([t["center_points"] for t in ts]).reshape(len(ts), n, 2),
            np.stack([t["area"] for t in ts]).reshape(len(ts), n))


def _run_targets(eng, labels, n, sp, shift, what, legacy=False):
    """One guarded call, then a second one over the poisoned outputs; both must equal the contract."""
    B, (h, w) = len(labels), labels.shape[1:]
    want = _want_targets(labels, n, sp, legacy)
    a = Arena(shift)
    d_lab = a.empty((B, h, w), torch.int32)
    d_lab.copy_(dev(labels))
    out = {"targets": a.empty((B, 6, h, w), torch.float32), "points": a.empty((B, n, 2), torch.float64), "area": a.empty((B, n), torch.int32)}
    for rnd in range(2):
        eng.loss_targets(d_lab, n, sp, out)
        torch.cuda.synchronize()
        assert a.intact(), f"{what}: wrote outside a tensor (call {rnd})"
        np.testing.assert_array_equal(d_lab.cpu().numpy(), labels, err_msg=what + ": the input changed")
        for k, wnt in zip(("targets", "points", "area"), want):
            got = out[k].cpu().numpy()
            np.testing.assert_array_equal(_bits(got), _bits(wnt.astype(got.dtype)), err_msg=f"{what}: {k} (call {rnd})")
        for t in out.values():
            t.view(torch.uint8).fill_(0xA7)                   # the second call starts from poisoned outputs


# ---- targets ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("path", golden_cases(), ids=lambda p: os.path.basename(p)[12:-4])
def test_targets_fixture_cases(path, shift):
    c = load_case(path)
    h, w = c["labels"].shape
    sp = Losses(sigma=c["sigma"], small_area=c["small_area"], small_weight=c["small_weight"])
    _run_targets(_engine(h, w), c["labels"][None], c["n"], sp, shift, os.path.basename(path))
    z = c["z"]                                               # ... and the recorded generator itself, not only its numpy statement
    got = _engine(h, w).loss_targets(dev(c["labels"][None]), c["n"], sp)["targets"][0].cpu().numpy()
    np.testing.assert_array_equal(_bits(got[0]), _bits(z["center"]))
    np.testing.assert_array_equal(_bits(got[1:3]), _bits(z["offset"]))
    np.testing.assert_array_equal(_bits(got[4]), _bits(z["sem_seg_weights"]))


@pytest.mark.parametrize("n", [1, 20, 254])
def test_targets_several_blocks(n):
    rng = np.random.default_rng(100 + n)
    lab = blob_labels(rng, 130, 200, n)                       # 26 000 pixels: tail words, seven paint blocks a frame
    _run_targets(_engine(130, 200), lab[None], n, Losses(sigma=6, small_area=300, small_weight=2.5), n % 2, f"130x200 n={n}")


def test_targets_three_frames_and_labels_out_of_range():
    rng = np.random.default_rng(7)
    labs = np.stack([blob_labels(rng, 130, 200, k) for k in (1, 20, 254)])
    labs[0, 5:9, 5:50] = 255                                  # out of 0..n_gt: none
    labs[1, 100:110, :] = -4
    labs[2, 0, :7] = 1 << 30
    _run_targets(_engine(130, 200), labs, 254, Losses(sigma=10, small_area=500), 0, "three frames")
    _run_targets(_engine(130, 200), labs[:2], 40, Losses(sigma=3, small_area=500), 1, "ids above n_gt")       # frame 1 holds ids up to 254


def test_targets_legacy_f32_and_the_widest_table():
    lab = blob_labels(np.random.default_rng(11), 37, 53, 9)
    _run_targets(_engine(37, 53, legacy=1), lab[None], 9, Losses(sigma=4, small_area=80), 0, "legacy f32", legacy=True)
    _run_targets(_engine(37, 53), lab[None], 9, Losses(sigma=20, small_area=80), 1, "sigma 20")


def test_targets_bad_arguments_refused():
    eng = _engine(37, 53)
    lib = _lib.load()
    lab = torch.zeros((1, 37, 53), dtype=torch.int32, device="cuda")
    g = torch.zeros((123 * 123,), dtype=torch.float32, device="cuda")
    t = torch.zeros((1, 6, 37, 53), dtype=torch.float32, device="cuda")
    pts, area = torch.zeros((1, 255, 2), dtype=torch.float64, device="cuda"), torch.zeros((1, 255), dtype=torch.int32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    for sigma, n in ((0, 3), (21, 3), (10, 255), (10, -1)):
        rc = lib.quber_loss_targets(eng.h, p(lab), 1, n, sigma, 10, 3.0, p(g), p(t), p(pts), p(area), None)
        assert rc != 0 and lib.quber_last_error(), (sigma, n)
    assert lib.quber_loss_targets(eng.h, p(lab), 4, 3, 10, 10, 3.0, p(g), p(t), p(pts), p(area), None) != 0       # batch > max_batch
    for bad in (dict(sigma=0), dict(sigma=21)):
        with pytest.raises(ValueError):
            Losses(**bad)


# ---- losses -----------------------------------------------------------------------------------------------------------------------------
def _to_losses(sp):
    kind = lambda h: sp.heads[h][1] if h in sp.heads else "dice"
    return (Losses(top_k=sp.top_k, foreground_weight=sp.foreground_weight, center_weight=sp.center_weight, offset_weight=sp.offset_weight,
                   error_type=sp.error_type, eee_mask_loss_type=kind("eee_mask"), eee_boundary_loss_type=kind("eee_boundary")),
            {h: first for h, (first, _) in sp.heads.items()})


def _close(got, want, what):
    assert got == pytest.approx(want, rel=REL, abs=ABS), what


def _check_frame(rec, ref, opts, heads, what):
    got, terms = opts.unpack(rec, heads)
    assert set(got) == set(ref["losses"]), what
    for k, v in ref["losses"].items():
        _close(got[k], v, f"{what}: {k}")
    rt = ref["terms"]
    for k in ("k", "kth", "above", "pixels"):
        assert terms[k] == rt[k], f"{what}: {k} {terms[k]!r} != {rt[k]!r}"          # selections and counts: exact
    for k in ("fg_sum", "center_num", "weight_sum", "offset_num"):
        _close(terms[k], rt[k], f"{what}: {k}")
    for h in heads:
        _close(terms[h]["ce_sum"], rt[h]["ce_sum"], f"{what}: {h} ce_sum")
        for k in ("inter", "target_sum", "prob_sum"):
            for g, w in zip(terms[h][k], rt[h][k]):
                _close(g, w, f"{what}: {h} {k}")


def _run_losses(eng, frames, sp, what):
    """frames: [(logits, targets dict or planes, explicit or None)] -> the records f64 [B,40], checked frame by frame."""
    opts, heads = _to_losses(sp)
    planes = [f[1] if isinstance(f[1], np.ndarray) else target_planes(f[1]) for f in frames]
    expl = dev(np.stack([f[2] for f in frames])) if heads else None
    out = eng.losses(dev(np.stack([f[0] for f in frames])), dev(np.stack(planes)), expl, opts, heads=heads)
    torch.cuda.synchronize()
    rec = out.cpu().numpy()
    assert np.isfinite(rec).all(), what
    for b, f in enumerate(frames):
        _check_frame(rec[b], losses_ref(f[0], planes[b], f[2], sp), opts, heads, f"{what} frame {b}")
    return out


LOSS_SPECS = {
    "plain": dict(),
    "dice_e3": dict(heads={"eee_boundary": (4, "dice")}),
    "ce_e3_two_heads": dict(heads={"eee_boundary": (4, "cross_entropy"), "eee_mask": (8, "cross_entropy")}),
    "e2_mixed": dict(error_type="e2", heads={"eee_boundary": (4, "cross_entropy"), "eee_mask": (6, "dice")}),
    "e33_mixed": dict(error_type="e33", heads={"eee_boundary": (4, "dice"), "eee_mask": (7, "cross_entropy")}),
    "e32_dice": dict(error_type="e32", heads={"eee_mask": (5, "dice"), "eee_boundary": (9, "dice")}),
}


@pytest.mark.parametrize("name", list(LOSS_SPECS))
@pytest.mark.parametrize("shape", [(37, 53), (96, 128), (130, 200)], ids=lambda s: "%dx%d" % s)
def test_losses_against_the_contract(shape, name):
    h, w = shape
    rng = np.random.default_rng(h * 7 + len(name))
    frames = [loss_inputs(rng, h, w, 12, scale=(1.0, 3.0, 8.0)[b], n=(0, 5, 30)[b]) for b in range(3)]         # batch 3; frame 0 has no instance
    for top_k in (1.0, 0.2, 1.0 / (h * w)):
        _run_losses(_engine(h, w), frames, spec(top_k=top_k, **LOSS_SPECS[name]), f"{name} {h}x{w} top_k={top_k:.3g}")


def test_losses_ties():
    h, w = 37, 53
    hw = h * w
    eng = _engine(h, w)
    empty = loss_targets_np(np.zeros((h, w), np.int32), 0, 2)             # t = 0, w = 1: the term is softplus(x), monotone in x
    const = np.full((4, h, w), 0.75, np.float32)
    x = np.full(hw, -1.0, np.float32)
    x[: hw // 10] = 2.0                                                   # 196 large values
    x[hw // 10: hw // 10 + hw * 3 // 10] = 0.5                            # a group of 588 equal ones; k = 392 falls inside it
    straddle = const.copy()
    straddle[0] = np.random.default_rng(0).permutation(x).reshape(h, w)
    for top_k in (0.2, 0.5, 1.0 / hw):
        rec = _run_losses(eng, [(const, empty, None), (straddle, empty, None)], spec(top_k=top_k), f"ties top_k={top_k:.3g}").cpu().numpy()
        if top_k == 0.2:                                      # the case is what it claims to be: the boundary lies inside the tie group
            assert rec[0, ls.W_ABOVE] == 0 and rec[1, ls.W_ABOVE] == hw // 10 < rec[1, ls.W_K] == int(0.2 * hw) < hw // 10 + hw * 3 // 10


def test_losses_large_logits_do_not_overflow():
    h, w = 37, 53
    rng = np.random.default_rng(9)
    logits, tg, explicit = loss_inputs(rng, h, w, 12)
    big = np.where(rng.random(logits.shape) < 0.5, np.float32(80), np.float32(-80))
    for top_k in (1.0, 0.2):
        _run_losses(_engine(h, w), [(big, tg, explicit), (logits, tg, explicit)],
                    spec(top_k=top_k, heads={"eee_boundary": (4, "dice"), "eee_mask": (8, "cross_entropy")}), "+-80")


def test_losses_bad_arguments_refused():
    eng = _engine(37, 53)
    logits, tg, explicit = loss_inputs(np.random.default_rng(1), 37, 53, 8)
    d_l, d_t, d_e = dev(logits[None]), dev(target_planes(tg)[None]), dev(explicit[None])
    with pytest.raises(ValueError):
        eng.losses(d_l, d_t, None, Losses(top_k=1.0 / (37 * 53 + 1)))                  # k == 0
    with pytest.raises(_lib.QuberError):
        eng.losses(d_l, d_t, d_e, Losses(), heads={"eee_mask": 6})                     # planes 6..9 of 8
    with pytest.raises(_lib.QuberError):
        eng.losses(d_l, d_t, d_e, Losses(), heads={"eee_mask": 2})
    with pytest.raises(ValueError):
        Losses(foreground_loss_type="cross_entropy")


# ---- determinism, footprint ---------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_equal():
    h, w = 130, 200
    rng = np.random.default_rng(21)
    frames = [loss_inputs(rng, h, w, 12, n=12) for _ in range(3)]
    eng = _engine(h, w)
    d_l, d_e = dev(np.stack([f[0] for f in frames])), dev(np.stack([f[2] for f in frames]))
    labs = dev(np.stack([blob_labels(rng, h, w, 12) for _ in range(3)]))
    opts = Losses(top_k=0.2, sigma=5, small_area=400)
    runs = []
    for _ in range(2):
        tg = eng.loss_targets(labs, 12, opts)
        rec = eng.losses(d_l, tg["targets"], d_e, opts, heads={"eee_boundary": 4, "eee_mask": 8})
        runs.append([t.clone() for t in (tg["targets"], tg["points"], tg["area"], rec)])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_an_engine_that_never_calls_the_feature_keeps_its_footprint():
    quiet, used = _engine(96, 128, tag="quiet"), _engine(96, 128, tag="used")
    base = quiet.workspace_bytes()
    assert used.workspace_bytes() == base                     # the same formula as before the feature: nothing of it in quber_create
    lab = dev(blob_labels(np.random.default_rng(2), 96, 128, 4)[None])
    tg = used.loss_targets(lab, 4)
    grown = used.workspace_bytes()
    assert grown > base
    used.losses(torch.zeros((1, 4, 96, 128), dtype=torch.float32, device="cuda"), tg["targets"], None, Losses(top_k=0.5))
    torch.cuda.synchronize()
    assert used.workspace_bytes() == grown and quiet.workspace_bytes() == base


# ---- predictor ----------------------------------------------------------------------------------------------------------------------------
PH, PW, PN = 96, 128, 3
POPTS = Losses(top_k=0.2, sigma=4, small_area=400, keep_targets=True)
_PCASE = []


def _pcase():
    """(two frames with PN masks each, their ground-truth label maps, random weights), computed once and left unchanged."""
    if not _PCASE:
        from quber_amd import arch, synth
        batch = synth.make_batch(5, 2, PH, PW, PN)
        rng = np.random.default_rng(8)
        _PCASE.append((batch, np.stack([blob_labels(rng, PH, PW, 4), blob_labels(rng, PH, PW, 6)]), arch.init_state_dict(seed=0)))
    return _PCASE[0]


def _predictor(**kw):
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
    return MaskRefinerPredictor(None, device="cuda:0", state_dict=_pcase()[2], **kw)


def _stream(pred, rgb, dep, masks, gts):
    hd = pred.model.enqueue_batch(dev(rgb), dev(dep), dev(masks), gt_labels=gts)
    return pred.model.collect_batch(hd)[0]


def _pass(pred, rgb, dep, masks, gts):
    """device_pass on buffers filled as predict_batch fills them -> (PassResult, dicts, upload_gt's triple)."""
    model, B = pred.model, len(rgb)
    gt = model.upload_gt(gts, B, PH, PW)
    eng = model.engine_for(PH, PW, 2 * B if model.tta else B, max(masks.shape[1], gt[2]))
    bgr, depth, d_masks = model.batch_buffers(B, PH, PW, masks.shape[1], True)
    bgr[:B].copy_(dev(rgb)), depth[:B].copy_(dev(dep)), d_masks[:B].copy_(dev(masks))
    rec = model.device_pass(eng, bgr, depth, d_masks, None, B, may_stop=True, gt=gt)
    return rec, model.results(rec, (bgr, depth)), gt


def _recomputed(rec, gt, opts):
    """Engine.loss_targets / error_maps / losses on the pass's own logits and masks -> (per-frame (losses, terms), targets, explicit)."""
    eng = rec.eng
    tg = eng.loss_targets(gt[0], gt[2], opts)
    heads = eng.loss_heads(opts)
    expl = eng.error_maps(rec.d_masks.contiguous(), gt[1])
    host = eng.losses(rec.logits, tg["targets"], expl, opts, heads=heads).cpu().numpy()
    return [opts.unpack(host[b], heads) for b in range(rec.B)], tg, expl


def _frames(batch):
    masks = (np.stack(batch["masks"]) != 0).astype(np.uint8) * np.uint8(255)
    return batch["rgb"], batch["depth"], masks


def test_predictor_paths_agree_and_equal_the_engine_calls():
    batch, gts, _ = _pcase()
    rgb, dep, masks = _frames(batch)
    pred = _predictor(losses=POPTS)
    try:
        one = pred.predict(rgb[0], dep[0], masks[0], gt_labels=gts[0])[0]
        assert set(one["losses"]) == {"loss_sem_seg", "loss_center", "loss_offset", "loss_eee_boundary"}
        for name, other in (("predict_batch", pred.predict_batch(rgb[:1], dep[:1], [masks[0]], gt_labels=gts[:1])[0]),
                            ("stream", _stream(pred, rgb[:1], dep[:1], masks[:1], gts[:1])[0])):
            assert other["losses"] == one["losses"] and other["loss_terms"] == one["loss_terms"], name
        two = pred.predict_batch(rgb, dep, [masks[0], masks[1]], gt_labels=list(gts))
        for b, other in enumerate(_stream(pred, rgb, dep, masks, gts)):
            assert other["losses"] == two[b]["losses"] and other["loss_terms"] == two[b]["loss_terms"], b
        rec, outs, gt = _pass(pred, rgb, dep, masks, gts)
        again, tg, expl = _recomputed(rec, gt, POPTS)
        sp = spec(top_k=POPTS.top_k, heads={"eee_boundary": (4, "dice")})
        for b in range(2):
            assert outs[b]["losses"] == two[b]["losses"] == again[b][0] and outs[b]["loss_terms"] == again[b][1]
            assert torch.equal(outs[b]["loss_targets"]["targets"], tg["targets"][b])
            want = loss_targets_np(gts[b], int(gts.max()), POPTS.sigma, POPTS.small_area, POPTS.small_weight)
            np.testing.assert_array_equal(_bits(outs[b]["loss_targets"]["targets"].cpu().numpy()), _bits(target_planes(want)))
            ref = losses_ref(rec.logits[b].cpu().numpy(), want, expl[b].cpu().numpy(), sp)          # ... and the contract on the same inputs
            for k, v in ref["losses"].items():
                _close(outs[b]["losses"][k], v, f"frame {b}: {k}")
            assert all(np.isfinite(v) and v > 0 for v in outs[b]["losses"].values())
    finally:
        pred.model.close()


def test_predictor_without_losses_or_ground_truth_changes_nothing():
    batch, gts, _ = _pcase()
    rgb, dep, masks = _frames(batch)
    pred = _predictor(losses=POPTS)
    try:
        eng = pred.model.engine_for(PH, PW, 2, PN)
        base = eng.workspace_bytes()
        plain = pred.predict_batch(rgb, dep, [masks[0], masks[1]])              # no gt_labels: nothing launched, nothing allocated
        assert eng.workspace_bytes() == base
        pred.model.losses = None
        off = pred.predict_batch(rgb, dep, [masks[0], masks[1]], gt_labels=list(gts))
        assert eng.workspace_bytes() == base
        pred.model.losses = POPTS
        on = pred.predict_batch(rgb, dep, [masks[0], masks[1]], gt_labels=list(gts))
        assert pred.model.engine_for(PH, PW, 2, PN).workspace_bytes() > base
        for b in range(2):
            assert set(plain[b]) == set(off[b]) == set(on[b]) - {"losses", "loss_terms", "loss_targets"}
            assert {"losses", "loss_terms", "loss_targets"} <= set(on[b])
            for key in ("sem_seg", "eee_boundary"):
                assert torch.equal(plain[b][key], on[b][key]) and torch.equal(off[b][key], on[b][key]), key
            assert torch.equal(plain[b]["panoptic_seg"][0], on[b]["panoptic_seg"][0])
    finally:
        pred.model.close()


def test_predictor_perturb_scores_the_masks_the_network_saw():
    from quber_amd.perturb import Perturb
    batch, gts, _ = _pcase()
    rgb, dep, masks = _frames(batch)
    pred = _predictor(losses=POPTS, perturb=Perturb(0.8, seed=3))
    try:
        rec, outs, gt = _pass(pred, rgb, dep, masks, gts)
        seen = torch.stack([o["perturbed_masks"] for o in outs])
        assert torch.equal(rec.d_masks, seen) and not torch.equal(seen, dev(masks))
        assert torch.equal(rec.ls["explicit"], rec.eng.error_maps(seen.contiguous(), gt[1]))
        assert not torch.equal(rec.ls["explicit"], rec.eng.error_maps(dev(masks), gt[1]))
        again, _, _ = _recomputed(rec, gt, POPTS)
        for b in range(2):
            assert outs[b]["losses"] == again[b][0]
    finally:
        pred.model.close()


def test_predictor_tta_scores_the_merged_logits():
    batch, gts, _ = _pcase()
    rgb, dep, masks = _frames(batch)
    pred = _predictor(losses=POPTS, tta=True)
    try:
        rec, outs, gt = _pass(pred, rgb, dep, masks, gts)
        assert rec.logits.shape[0] == 2 and rec.eng.qcfg.max_batch >= 4          # the merged logits of the 2 frames, from a forward of 4
        again, _, _ = _recomputed(rec, gt, POPTS)
        for b in range(2):
            assert outs[b]["losses"] == again[b][0]
            assert torch.equal(outs[b]["sem_seg"], rec.logits[b, 0:1])
    finally:
        pred.model.close()


def test_predictor_refuses_iterations_and_zoom():
    from quber_amd.maskrefiner.predictor import RefineOptions
    from quber_amd.zoom import ZoomIn
    for kw in (dict(iterations=2), dict(zoom=ZoomIn(crop=32))):
        with pytest.raises(ValueError, match="losses"):
            RefineOptions.parse(losses=POPTS, **kw)
        with pytest.raises(ValueError, match="losses"):
            _predictor(losses=POPTS, **kw)
    with pytest.raises(ValueError):
        RefineOptions.parse(losses="dice")
