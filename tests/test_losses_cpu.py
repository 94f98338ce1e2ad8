"""CPU: the contract of the validation losses (csrc/losses.hip; INTEGRATION.md "Validation losses") - loss_targets_np, the numpy statement
of the reference's PanopticDeepLabTargetGenerator (maskrefiner/data/dataset_mappers/target_generator.py:8-165) for datasets whose segments
are all things and none crowd, and losses_ref, the five values of the reference's loss dict (maskrefiner/modeling/mask_refiner/model.py:36-72,
:672-687, :766-802) per frame, in float64 torch on the CPU.  tests/test_gpu_losses.py holds the device to both.

loss_targets_np is pinned bit for bit by tests/golden/losstargets_*.npz, recorded from the reference's own generator (tools/gen_loss_golden.py).
The five terms are pinned against torch's own modules composed here (BCEWithLogitsLoss, topk, MSELoss, L1Loss, softmax, CrossEntropyLoss).

Stated deviations (INTEGRATION.md has them in words):
  * values are PER FRAME: the reference's value for a batch holding that one frame.  Its batch-level top-k (one selection over all frames'
    pixels) and batch-level dice mean are not reproduced; `terms` holds the raw pieces from which the centre / offset / cross-entropy values
    of a multi-frame batch recompose;
  * nn.CrossEntropyLoss refuses the reference's `long` same-shape targets (torch 2.10: "Expected floating point type for target with class
    probabilities, got Long"); the contract is the .float() cast that makes the reference's line run;
  * MONAI is not installed here: the dice term restates DiceLoss(softmax=True) from the copy in the reference's
    explicit_error_estimation/loss.py:95-160 (smooth_nr = smooth_dr = 1e-5, mean over classes) and is argued, not run against MONAI;
  * foreground_loss_type "cross_entropy" is refused: the reference's one-plane foreground head cannot run it either;
  * top_k == 1.0 selects nothing: kth and above are reported as 0.
"""
import glob
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERROR_CLASSES = {"e3": 4, "e2": 2, "e33": 3, "e32": 2}
LOSS_KEYS = ("loss_sem_seg", "loss_center", "loss_offset", "loss_eee_mask", "loss_eee_boundary")
HEAD_KIND = {"eee_mask": 0, "eee_boundary": 1}           # plane of the explicit maps [2 (region, boundary)][4 (TP, TN, FP, FN)]
DICE_SMOOTH = 1e-5


# ---- the contract: targets ----------------------------------------------------------------------------------------------------------------
def gauss_table(sigma):
    """target_generator.py:46-51: exp in float64, then float32.  The reference keeps the float64 table, takes np.maximum(f32 centre, f64
    table) and stores the float64 result into the float32 centre plane: max, then round.  Rounding to float32 is monotone (a <= b implies
    f32(a) <= f32(b)) and leaves a float32 unchanged, so that equals the maximum of the ROUNDED values - one float32 table serves."""
    size, c = 6 * sigma + 3, 3 * sigma + 1
    x = np.arange(size, dtype=np.float64)
    return np.exp(-((x - c) ** 2 + (x[:, None] - c) ** 2) / (2 * sigma ** 2)).astype(np.float32)


def loss_targets_np(gt_labels, n, sigma=10, small_area=4096, small_weight=3, legacy_f32=False):
    """gt_labels int [H,W] (0 = none, 1..n; any other value counts as 0) -> dict of center f32 [H,W], offset f32 [2,H,W] (y, x), sem_seg u8,
    sem_seg_weights f32, inst_weights u8 (the reference's center_weights == offset_weights), center_points f64 [n,2] (y, x; zeros for an
    id without a pixel) and area i32 [n].  legacy_f32: the offsets as numpy < 2 computes `float64 scalar - float32 array` (all float32)."""
    lab = np.asarray(gt_labels).astype(np.int64)
    lab = np.where((lab >= 1) & (lab <= n), lab, 0)
    H, W = lab.shape
    g = gauss_table(sigma)
    center = np.zeros((H, W), np.float32)
    offset = np.zeros((2, H, W), np.float32)
    weights = np.ones((H, W), np.float32)
    points = np.zeros((n, 2), np.float64)
    area = np.zeros((n,), np.int32)
    for i in range(1, n + 1):
        ys, xs = np.nonzero(lab == i)
        if not len(ys):
            continue
        area[i - 1] = len(ys)
        if len(ys) < small_area:
            weights[ys, xs] = small_weight
        cy, cx = np.float64(int(ys.sum())) / np.float64(len(ys)), np.float64(int(xs.sum())) / np.float64(len(xs))
        points[i - 1] = (cy, cx)
        y, x = int(round(cy)), int(round(cx))                      # ties to even
        ux, uy, bx, by = x - 3 * sigma - 1, y - 3 * sigma - 1, x + 3 * sigma + 2, y + 3 * sigma + 2
        x0, x1, y0, y1 = max(0, ux), min(bx, W), max(0, uy), min(by, H)
        center[y0:y1, x0:x1] = np.maximum(center[y0:y1, x0:x1], g[y0 - uy:y1 - uy, x0 - ux:x1 - ux])
        if legacy_f32:
            offset[0, ys, xs] = np.float32(cy) - ys.astype(np.float32)
            offset[1, ys, xs] = np.float32(cx) - xs.astype(np.float32)
        else:
            offset[0, ys, xs] = (cy - ys.astype(np.float64)).astype(np.float32)
            offset[1, ys, xs] = (cx - xs.astype(np.float64)).astype(np.float32)
    fg = (lab != 0).astype(np.uint8)
    return {"center": center, "offset": offset, "sem_seg": fg, "sem_seg_weights": weights, "inst_weights": fg.copy(), "center_points": points,
            "area": area}


def target_planes(t):
    """The dict of loss_targets_np -> f32 [6,H,W] in the device's plane order: center, off_y, off_x, sem_seg, sem_seg_weights, inst_weights."""
    return np.stack([t["center"], t["offset"][0], t["offset"][1], t["sem_seg"].astype(np.float32), t["sem_seg_weights"],
                     t["inst_weights"].astype(np.float32)]).astype(np.float32)


# ---- the contract: losses -----------------------------------------------------------------------------------------------------------------
def spec(top_k=1.0, foreground_weight=1.0, center_weight=200.0, offset_weight=0.01, error_type="e3", heads=None,
         foreground_loss_type="hard_pixel_mining"):
    """heads: {"eee_boundary" | "eee_mask": (first logit plane, "dice" | "cross_entropy")}."""
    return types.SimpleNamespace(top_k=top_k, foreground_weight=foreground_weight, center_weight=center_weight, offset_weight=offset_weight,
                                 error_type=error_type, heads=dict(heads or {}), foreground_loss_type=foreground_loss_type)


def top_k_pixels(top_k, numel):
    """model.py:70.  0 is refused: the reference would take the mean of nothing (NaN)."""
    k = numel if top_k == 1.0 else int(top_k * numel)
    if k < 1:
        raise ValueError("top_k * H * W < 1: no pixel would be selected")
    return k


def topk_sum(values, k):
    """values: non-negative float64, flat -> (sum of the k largest, the k-th largest T, #{v > T}) as sum_{v > T} v + (k - #{v > T}) * T:
    the values tied at T are equal by definition, so which of them a selection takes does not matter."""
    v = torch.sort(values.reshape(-1), descending=True).values
    T = v[k - 1]
    above = int((v > T).sum())
    return float(v[:above].sum() + (k - above) * T), float(T), above


def eee_targets(explicit_kind, error_type):
    """explicit_kind u8 [4,H,W] (TP, TN, FP, FN) -> float64 [C,H,W]: the target stack of model.py:186-226, sums as written there."""
    tp, tn, fp, fn = (torch.as_tensor(np.asarray(explicit_kind) != 0).to(torch.float64)[i] for i in range(4))
    return torch.stack({"e3": (tp, tn, fp, fn), "e2": (tp + tn, fp + fn), "e33": (tp + tn, fp, fn), "e32": (fp, fn)}[error_type])


def losses_ref(logits, targets, explicit, sp):
    """logits f32 [P,H,W], targets f32 [6,H,W] (target_planes) or the dict of loss_targets_np, explicit u8 [2,4,H,W] or None, sp: spec()
    -> {"losses": {key: float}, "terms": {...}} of ONE frame, float64."""
    if sp.foreground_loss_type != "hard_pixel_mining":
        raise ValueError("foreground_loss_type %r: only hard_pixel_mining (the one-plane foreground head cannot run cross_entropy)" % sp.foreground_loss_type)
    if isinstance(targets, dict):
        targets = target_planes(targets)
    x = torch.as_tensor(np.asarray(logits)).to(torch.float64)
    t = torch.as_tensor(np.asarray(targets)).to(torch.float64)
    hw = x.shape[1] * x.shape[2]
    k = top_k_pixels(sp.top_k, hw)
    fg = torch.clamp(x[0], min=0) - x[0] * t[3] + torch.log1p(torch.exp(-x[0].abs()))
    fg = fg * t[4]
    if sp.top_k == 1.0:
        fg_sum, kth, above = float(fg.sum()), 0.0, 0
    else:
        fg_sum, kth, above = topk_sum(fg, k)
    w = t[5]
    wsum = float(w.sum())
    c_num = float((((x[1] - t[0]) ** 2) * w).sum())
    o_num = float(((x[2:4] - t[1:3]).abs() * w[None]).sum())
    out = {"loss_sem_seg": sp.foreground_weight * fg_sum / k,
           "loss_center": sp.center_weight * c_num / wsum if wsum > 0 else 0.0,
           "loss_offset": sp.offset_weight * o_num / wsum if wsum > 0 else 0.0}          # one-plane weight sum under two planes: model.py:796-798
    terms = {"fg_sum": fg_sum, "k": k, "kth": kth, "above": above, "center_num": c_num, "weight_sum": wsum, "offset_num": o_num, "pixels": hw}
    for head, (first, kind) in sp.heads.items():
        C = ERROR_CLASSES[sp.error_type]
        tg = eee_targets(np.asarray(explicit)[HEAD_KIND[head]], sp.error_type)
        z = x[first:first + C]
        logp = z - torch.logsumexp(z, 0, keepdim=True)
        p = torch.exp(logp)
        ce = float(-(tg * logp).sum())
        inter, tsum, psum = (tg * p).sum((1, 2)), tg.sum((1, 2)), p.sum((1, 2))
        if kind == "dice":
            val = float((1.0 - (2.0 * inter + DICE_SMOOTH) / (tsum + psum + DICE_SMOOTH)).mean())
        elif kind == "cross_entropy":
            val = ce / hw
        else:
            raise ValueError("loss type %r" % (kind,))
        out["loss_" + head] = val
        terms[head] = {"ce_sum": ce, "inter": inter.tolist(), "target_sum": tsum.tolist(), "prob_sum": psum.tolist()}
    return {"losses": out, "terms": terms}


# ---- cases shared with tests/test_gpu_losses.py -------------------------------------------------------------------------------------------
def golden_cases():
    files = sorted(glob.glob(os.path.join(GOLDEN, "losstargets_*.npz")))
    assert files, "no golden fixtures losstargets_*.npz"
    return files


def load_case(path):
    z = np.load(path)
    sigma, n, small_area, small_weight = (int(v) for v in z["params"])
    return {"labels": z["labels"].astype(np.int32), "n": n, "sigma": sigma, "small_area": small_area, "small_weight": small_weight, "z": z}


def blob_labels(rng, h, w, n, declared=None):
    """A label map of n random boxes / discs painted over one another (later over earlier; some ids may end without a pixel)."""
    lab = np.zeros((h, w), np.int32)
    yy, xx = np.mgrid[:h, :w]
    for i in range(1, n + 1):
        cy, cx, ry, rx = rng.integers(0, h), rng.integers(0, w), rng.integers(1, max(2, h // 3)), rng.integers(1, max(2, w // 3))
        m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1 if i % 2 else (abs(yy - cy) <= ry) & (abs(xx - cx) <= rx)
        lab[m] = i
    return lab


def loss_inputs(rng, h, w, planes, scale=3.0, n=5):
    """(logits f32 [planes,h,w], targets dict, explicit u8 [2,4,h,w]) of one random frame."""
    lab = blob_labels(rng, h, w, n)
    tg = loss_targets_np(lab, n, sigma=4, small_area=h * w // 8, small_weight=3)
    logits = (rng.standard_normal((planes, h, w)) * scale).astype(np.float32)
    cls = rng.integers(0, 4, (2, h, w))
    explicit = (cls[:, None] == np.arange(4)[None, :, None, None]).astype(np.uint8)
    return logits, tg, explicit


# ---- tests: targets -----------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("path", golden_cases(), ids=lambda p: os.path.basename(p)[12:-4])
def test_targets_equal_the_recorded_generator(path):
    c = load_case(path)
    z = c["z"]
    got = loss_targets_np(c["labels"], c["n"], c["sigma"], c["small_area"], c["small_weight"], legacy_f32=False)
    for key in ("center", "offset", "sem_seg_weights"):
        np.testing.assert_array_equal(_bits(got[key]), _bits(z[key].astype(np.float32)), err_msg=key)
    np.testing.assert_array_equal(got["sem_seg"], z["sem_seg"])
    np.testing.assert_array_equal(got["inst_weights"], z["center_weights"])
    np.testing.assert_array_equal(got["inst_weights"], z["offset_weights"])
    np.testing.assert_array_equal(got["area"], z["area"])
    present = got["area"] > 0
    np.testing.assert_array_equal(_bits(got["center_points"][present]), _bits(z["center_points"].reshape(-1, 2)))
    assert not got["center_points"][~present].any()


def test_fixture_cases_cover_the_edges():
    cases = {os.path.basename(p)[12:-4]: load_case(p) for p in golden_cases()}
    c = cases["clip_37x53_s10"]
    t = loss_targets_np(c["labels"], c["n"], c["sigma"], c["small_area"], c["small_weight"])
    assert c["labels"].shape == (37, 53) and c["sigma"] == 10 and (t["center"] > 0).all()          # 63 > 53, 37: clipped on all four sides
    assert cases["scene_96x128_s8"]["labels"].shape == (96, 128) and cases["scene_96x128_s8"]["sigma"] == 8
    assert any(c["sigma"] == 1 for c in cases.values())
    c = cases["ties_20x24_s2"]
    t = loss_targets_np(c["labels"], c["n"], c["sigma"], c["small_area"], c["small_weight"])
    frac = t["center_points"] % 1.0
    assert (t["area"] == 2).all() and (frac == 0.5).any(1).all()
    halves = np.floor(t["center_points"][frac == 0.5]).astype(int)
    assert (halves % 2 == 0).any() and (halves % 2 == 1).any()                                  # x.5 below an odd and below an even integer
    c = cases["small_64x96_s4"]
    t = loss_targets_np(c["labels"], c["n"], c["sigma"], c["small_area"], c["small_weight"])
    assert sorted(t["area"].tolist())[:2] == [c["small_area"] - 1, c["small_area"]]
    assert set(np.unique(t["sem_seg_weights"]).tolist()) == {1.0, float(c["small_weight"])}
    c = cases["absent_32x48_s3"]
    assert (loss_targets_np(c["labels"], c["n"], c["sigma"])["area"] == 0).any()
    assert cases["empty_16x16_s2"]["n"] == 0
    c = cases["overlap_40x60_s5"]
    t = loss_targets_np(c["labels"], c["n"], c["sigma"], c["small_area"], c["small_weight"])
    singles = [loss_targets_np(np.where(c["labels"] == i, i, 0), c["n"], c["sigma"])["center"] for i in range(1, c["n"] + 1)]
    assert ((singles[0] > 0) & (singles[1] > 0)).any()                                          # the windows overlap ...
    np.testing.assert_array_equal(t["center"], np.maximum.reduce(singles))                     # ... and the maximum decides
    assert (singles[0] > singles[1]).any() and (singles[1] > singles[0]).any()


def test_legacy_f32_offsets_differ_by_the_rounding_of_the_centre():
    rng = np.random.default_rng(5)
    lab = blob_labels(rng, 61, 83, 7)
    a, b = loss_targets_np(lab, 7, 4, legacy_f32=False), loss_targets_np(lab, 7, 4, legacy_f32=True)
    for key in ("center", "sem_seg", "sem_seg_weights", "inst_weights", "center_points", "area"):
        np.testing.assert_array_equal(a[key], b[key])
    d = np.abs(a["offset"].astype(np.float64) - b["offset"].astype(np.float64))
    assert d.max() > 0, "the two modes agree everywhere: the case does not exercise the split"
    assert d.max() <= np.spacing(np.float32(83))                   # the centre rounded to float32, then one more float32 rounding
    for i in range(1, 8):                                           # mode 1 is the all-float32 expression, mode 0 the float64 one rounded once
        ys, xs = np.nonzero(lab == i)
        if len(ys):
            cy = a["center_points"][i - 1, 0]
            np.testing.assert_array_equal(b["offset"][0, ys, xs], np.float32(cy) - ys.astype(np.float32))
            np.testing.assert_array_equal(a["offset"][0, ys, xs], (cy - ys).astype(np.float32))


def test_labels_out_of_range_count_as_none():
    lab = np.array([[0, 1, 1, 9], [-3, 2, 2, 3]], np.int32)
    t = loss_targets_np(lab, 2, 1)
    np.testing.assert_array_equal(t["sem_seg"], [[0, 1, 1, 0], [0, 1, 1, 0]])
    np.testing.assert_array_equal(t["area"], [2, 2])


# ---- tests: losses ------------------------------------------------------------------------------------------------------------------------
def _torch_composition(logits, tg, explicit, sp, dtype):
    """The reference's lines on torch's own modules, in `dtype`, for a batch of this one frame."""
    x = torch.as_tensor(logits).to(dtype)[None]
    t = {k: torch.as_tensor(v).to(dtype) for k, v in tg.items() if k not in ("center_points", "area")}
    px = nn.BCEWithLogitsLoss(reduction="none")(x[:, 0], t["sem_seg"][None]) * t["sem_seg_weights"][None]          # model.py:59-66
    px = px.contiguous().view(-1)
    if sp.top_k == 1.0:
        fg = px.mean()
    else:
        fg = torch.topk(px, int(sp.top_k * px.numel())).values.mean()
    w = t["inst_weights"][None, None]
    c = nn.MSELoss(reduction="none")(x[:, 1:2], t["center"][None, None]) * w
    o = nn.L1Loss(reduction="none")(x[:, 2:4], t["offset"][None]) * w
    out = {"loss_sem_seg": float(fg * sp.foreground_weight),
           "loss_center": float((c.sum() / w.sum() if w.sum() > 0 else c.sum() * 0) * sp.center_weight),
           "loss_offset": float((o.sum() / w.sum() if w.sum() > 0 else o.sum() * 0) * sp.offset_weight)}
    for head, (first, kind) in sp.heads.items():
        C = ERROR_CLASSES[sp.error_type]
        z = x[:, first:first + C]
        y = eee_targets(explicit[HEAD_KIND[head]], sp.error_type).to(dtype)[None]
        if kind == "cross_entropy":
            out["loss_" + head] = float(nn.CrossEntropyLoss(reduction="mean")(z, y))
        else:                                                      # DiceLoss(softmax=True): loss.py:111, 139-156
            p = torch.softmax(z, 1)
            inter, den = torch.sum(y * p, dim=[2, 3]), torch.sum(y, dim=[2, 3]) + torch.sum(p, dim=[2, 3])
            out["loss_" + head] = float(torch.mean(1.0 - (2.0 * inter + DICE_SMOOTH) / (den + DICE_SMOOTH)))
    return out


SPECS = [spec(), spec(top_k=0.2, heads={"eee_boundary": (4, "dice")}),
         spec(top_k=0.2, error_type="e2", heads={"eee_boundary": (4, "cross_entropy"), "eee_mask": (6, "dice")}),
         spec(top_k=0.5, error_type="e33", heads={"eee_boundary": (4, "dice"), "eee_mask": (7, "cross_entropy")}),
         spec(error_type="e32", heads={"eee_mask": (4, "dice"), "eee_boundary": (6, "cross_entropy")})]


@pytest.mark.parametrize("i", range(len(SPECS)))
def test_losses_ref_equals_the_torch_composition(i):
    sp = SPECS[i]
    logits, tg, explicit = loss_inputs(np.random.default_rng(10 + i), 37, 53, 12)
    got = losses_ref(logits, tg, explicit, sp)["losses"]
    f64, f32 = _torch_composition(logits, tg, explicit, sp, torch.float64), _torch_composition(logits, tg, explicit, sp, torch.float32)
    assert set(got) == set(f64) == {"loss_sem_seg", "loss_center", "loss_offset"} | {"loss_" + h for h in sp.heads}
    for key in got:
        assert got[key] == pytest.approx(f64[key], rel=1e-12, abs=1e-300), key
        assert got[key] == pytest.approx(f32[key], rel=2e-5), key        # float32 sums of 1961 terms: a few hundred ulp at the very most


def test_topk_sum_equals_torch_topk():
    rng = np.random.default_rng(3)
    v = torch.as_tensor(rng.random(1000))
    tie = torch.cat([torch.full((7,), 0.9), torch.full((10,), 0.5), torch.as_tensor(rng.random(20) * 0.4)]).to(torch.float64)
    for vals, k in ((v, 1), (v, 200), (v, 1000), (torch.full((64,), 0.25, dtype=torch.float64), 13), (tie, 12), (tie, 7), (tie, 17), (tie, 18)):
        s, T, above = topk_sum(vals, k)
        top = torch.topk(vals, k).values
        assert s / k == pytest.approx(float(top.mean()), rel=1e-14)
        assert T == float(top[-1]) and above == int((vals > T).sum()) and above < k
    assert topk_sum(tie, 12)[1:] == (0.5, 7)                       # the boundary falls inside the group of ten tied values


def test_offset_denominator_is_the_one_plane_weight_sum():
    logits, tg, _ = loss_inputs(np.random.default_rng(1), 20, 30, 4)
    r = losses_ref(logits, tg, None, spec(offset_weight=1.0))
    w = tg["inst_weights"].astype(np.float64)
    both = np.abs(logits[2:4].astype(np.float64) - tg["offset"]) * w[None]
    assert r["losses"]["loss_offset"] == pytest.approx(both.sum() / w.sum(), rel=1e-13)
    assert r["losses"]["loss_offset"] == pytest.approx(2 * both.sum() / np.broadcast_to(w[None], both.shape).sum(), rel=1e-13)
    assert r["terms"]["weight_sum"] == w.sum()


def test_zero_weight_frame_gives_zero():
    logits = np.random.default_rng(2).standard_normal((4, 16, 16)).astype(np.float32)
    r = losses_ref(logits, loss_targets_np(np.zeros((16, 16), np.int32), 0, 2), None, spec())
    assert r["losses"]["loss_center"] == 0.0 and r["losses"]["loss_offset"] == 0.0 and r["losses"]["loss_sem_seg"] > 0
    assert r["terms"]["weight_sum"] == 0.0


def test_error_type_target_stacks():
    e = np.zeros((4, 1, 4), np.uint8)
    e[np.arange(4), 0, np.arange(4)] = 1                           # pixel i is TP, TN, FP, FN
    want = {"e3": np.eye(4), "e2": [[1, 1, 0, 0], [0, 0, 1, 1]], "e33": [[1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], "e32": [[0, 0, 1, 0], [0, 0, 0, 1]]}
    for et, w in want.items():
        got = eee_targets(e, et).numpy()[:, 0]
        np.testing.assert_array_equal(got, np.asarray(w, np.float64), err_msg=et)
        assert got.shape[0] == ERROR_CLASSES[et]
    assert (eee_targets(e, "e32").sum(0) == 0).any()               # a pixel may have no class
    from quber_amd.eval import error_maps as em
    for et in want:                                                # the same stacks as the scorer's class map (quber_error_score)
        cls = em.target_class_map(e, et)
        st = eee_targets(e, et).numpy()
        np.testing.assert_array_equal(np.where(st.sum(0) > 0, st.argmax(0), ERROR_CLASSES[et]), cls)


def test_refusals():
    logits, tg, _ = loss_inputs(np.random.default_rng(4), 8, 8, 4)
    with pytest.raises(ValueError):
        losses_ref(logits, tg, None, spec(foreground_loss_type="cross_entropy"))
    with pytest.raises(ValueError):
        losses_ref(logits, tg, None, spec(top_k=1.0 / 65))          # k == 0
    assert losses_ref(logits, tg, None, spec(top_k=1.0 / 64))["terms"]["k"] == 1


def test_losses_record_and_config_defaults():
    from quber_amd.losses import Losses
    d = Losses()
    assert (d.sigma, d.small_area, d.small_weight, d.top_k) == (10, 4096, 3, 1.0)
    assert (d.foreground_weight, d.center_weight, d.offset_weight) == (1.0, 200.0, 0.01)
    assert d.eee_mask_loss_type == d.eee_boundary_loss_type == "dice" and d.error_type == "e3"
    assert Losses.from_cfg(None) == d
    for bad in (dict(sigma=0), dict(sigma=21), dict(top_k=0.0), dict(top_k=1.5), dict(eee_mask_loss_type="focal"), dict(error_type="e4"),
                dict(foreground_loss_type="cross_entropy")):
        with pytest.raises(ValueError):
            Losses(**bad)
    assert Losses.parse(None) is None and Losses.parse(d) is d
    with pytest.raises(ValueError):
        Losses.parse("dice")
