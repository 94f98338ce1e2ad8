"""CPU: the scene-level perturbation (INTEGRATION.md "Scene-level perturbation"; csrc/scene.hip, quber_amd/scene.py).

The contract in numpy (``scene_perturb_np`` on the tables of ``quber_amd.scene.scene_draws``: tests/test_gpu_scene.py compares the HIP
path against it - masks, info and report alike, exactly), a description of the reference's stage in the reference's own dtypes
(``reference_scene``: tools/ours/perturbate_masks.py:101-205 - 0 / 1 uint8 ground truth and proposals, a 0 / 255 list, ``compute_iou``'s
``seg * gt`` / ``seg + gt`` counting in uint8, the ``mask != 1`` box, coins read from the same tables) which must give the same mask
lists on seeded random scenes, hand-drawn cases for every rule, the order of ``scene_draws``, the ``ScenePerturb`` validation, the ABI
entry and the scenes the GPU tests run.

The contract is stated on pixel sets.  The ONE uint8 wrap of the reference it reproduces is in step 3: ``compute_iou(gt_mask,
perturbated_mask)`` adds a 0 / 1 mask to a 0 / 255 mask, 1 + 255 wraps to 0, so the "union" it counts is the symmetric difference.  The
wraps it does NOT reproduce: after a merge the pixels where the two masks overlap hold 255 + 255 = 254 (and 253, ... after more), so the
byte sums a split compares with the area limit are a few units below 255 x pixels; and ``dilated * mask2`` is 0 where both bytes are
multiples of 16, which takes a 16-fold overlap of merged masks.  The contract counts 255 per pixel and tests sets.

OpenCV is not installed here, so the agreement of ``dilate10`` with ``cv2.dilate(mask, np.ones((10, 10), np.uint8))`` is ARGUED from
OpenCV's documentation - ``dst(x, y) = max over the element's (x', y') of src(x + x' - anchor.x, y + y' - anchor.y)``, the default anchor
at the element's centre ``(cols / 2, rows / 2) = (5, 5)``, the default constant border that reads as 0 for a dilation - and is not
tested: an output pixel x sees the inputs x - 5 .. x + 4, i.e. a set pixel spreads 5 to the right and below, 4 to the left and above."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from quber_amd import _lib
from quber_amd.scene import ATTEMPTS, DEFAULT_RANGES, MAX_SLOTS, ScenePerturb, scene_draws

REPORT = ("count", "n_fp", "n_gs", "gt_kept", "absorbed", "splits", "deleted", "dropped")


# ---- the contract ----
def dilate10(e):
    """e bool [h, w] -> dilate10(e)(y, x) = OR over i, j in 0..9 of e(y + i - 5, x + j - 5), 0 outside the frame."""
    h, w = e.shape
    p = np.zeros((h + 10, w + 10), bool)
    p[5:5 + h, 5:5 + w] = e
    out = np.zeros((h, w), bool)
    for i in range(10):
        for j in range(10):
            out |= p[i:i + h, j:j + w]           # p(y + i, x + j) = e(y + i - 5, x + j - 5)
    return out


def cut_region(h, w, x1, y1, axis, side):
    """The pixels a split attempt cuts off, bool [h, w].  x1 / y1 are clipped to the frame (a table of scene_draws never needs it); the
    last row and the last column are never cut."""
    x1, y1 = min(max(int(x1), 0), w - 1), min(max(int(y1), 0), h - 1)
    c = np.zeros((h, w), bool)
    if axis == 0:
        if side == 0:
            c[y1:h - 1] = True
        else:
            c[:y1] = True
    else:
        if side == 0:
            c[:, x1:w - 1] = True
        else:
            c[:, :x1] = True
    return c


def scene_perturb_np(gt, props, n_gt, n_prop, M, min_mask_ratio, d, stats=None):
    """One frame.  gt [N,h,w], props [P,h,w] (non-zero = inside; only the first n_gt / n_prop rows are read), the capacity M, d: the
    tables of scene_draws (fp_act, gs_act [>= n_prop]; merge_act, split_act, delete_act [M]; split_try [M,10,4]) ->
    (masks u8 [M,h,w] of 0 / 255, zero planes behind count; info i32 [M,4]: kind (0 ground truth, 1 false positive, 2 over- / under-
    segmentation), the source index of the slot's own origin, the number of members, split (0 none, 1 the kept half, 2 the cut-off
    half), zero rows behind count; report i32 [8]: count, n_fp, n_gs, ground truths kept, absorbed, splits, deleted, dropped).
    stats: a dict that receives counts of the branches taken (the tests assert that their scenes reach every one)."""
    gt, props = np.asarray(gt), np.asarray(props)
    h, w = (gt if gt.ndim == 3 else props).shape[1:]
    G = [gt[g] != 0 for g in range(n_gt)]
    Q = [props[q] != 0 for q in range(n_prop)]
    cnt = np.count_nonzero
    lim = np.float64(w * h) * min_mask_ratio
    st = stats if stats is not None else {}
    bump = lambda key, by=1: st.__setitem__(key, st.get(key, 0) + by)

    def iou(a, b):
        return (cnt(a & b) + 1e-6) / (cnt(a | b) + 1e-6)

    L, rep = [], dict.fromkeys(REPORT, 0)

    def append(plane, kind, src, members=1, split=0):
        if len(L) >= M:
            rep["dropped"] += 1
            return False
        L.append({"plane": plane, "kind": kind, "src": src, "members": members, "split": split})
        return True

    # 1. false positives
    max_gt = max([cnt(g) for g in G] + [0])
    for q in range(n_prop):
        if not d["fp_act"][q]:
            continue
        a = cnt(Q[q])
        if a < lim or a > 2.0 * max_gt:
            continue
        max_iou = 0.0
        for g in G:
            max_iou = max(max_iou, iou(g, Q[q]))
        if max_iou < 0.3 and append(Q[q], 1, q):
            rep["n_fp"] += 1
    # 2. over- and under-segmentation
    for q in range(n_prop):
        if not d["gs_act"][q] or cnt(Q[q]) < lim:
            continue
        max_iou = 0.0
        for g in G:
            max_iou = max(max_iou, iou(g, Q[q]))
        if max_iou > 0.3 and append(Q[q], 2, q):
            rep["n_gs"] += 1
    # 3. the ground truths no entry covers; the denominator is the symmetric difference (the reference's 1 + 255 wraps to 0)
    entries = [e["plane"] for e in L]
    for g in range(n_gt):
        max_iou = true_iou = 0.0
        for e in entries:
            inter, union = cnt(G[g] & e), cnt(G[g] | e)
            max_iou = max(max_iou, (inter + 1e-6) / ((union - inter) + 1e-6))
            true_iou = max(true_iou, (inter + 1e-6) / (union + 1e-6))
        if (max_iou < 0.3) != (true_iou < 0.3):
            bump("wrapped_union_decides")
        if max_iou < 0.3:
            if append(G[g], 0, g):
                rep["gt_kept"] += 1
        else:
            bump("gt_replaced")
    # 4. merge: logic on the L1 x L1 touch table (dilation and intersection distribute over unions)
    L1 = len(L)
    dil = [dilate10(e["plane"]) for e in L]
    touch = [[bool((dil[a] & L[b]["plane"]).any()) for b in range(L1)] for a in range(L1)]
    S = [{k} for k in range(L1)]
    for idx1 in range(L1):
        if not d["merge_act"][idx1]:
            continue
        A = set(S[idx1])                             # the reference reads mask1 once
        if not A:
            bump("absorbed_before_own_turn")
        hits = 0
        for idx2 in range(L1):
            if idx2 == idx1:
                continue
            if any(touch[a][b] for a in A for b in S[idx2]):
                S[idx1] = A | S[idx2]                # replaces: of several touching masks only the last stays merged
                S[idx2] = set()
                hits += 1
        rep["absorbed"] += hits
        if hits > 1:
            bump("multi_absorption_merges")
            bump("multi_absorptions", hits)
    merged = []
    for k in range(L1):
        plane = np.zeros((h, w), bool)
        for m in S[k]:
            plane |= L[m]["plane"]
        if plane.any():
            merged.append(dict(L[k], plane=plane, members=len(S[k])))
    L = merged
    # 5. split; appended halves are not revisited
    L2 = len(L)
    for idx in range(L2):
        if not d["split_act"][idx]:
            continue
        e = L[idx]["plane"]
        for k in range(ATTEMPTS):
            x1, y1, axis, side = (int(v) for v in d["split_try"][idx][k])
            c = cut_region(h, w, x1, y1, axis, side)
            m1, m2 = e & ~c, e & c
            if 255.0 * cnt(m1) >= lim and 255.0 * cnt(m2) >= lim:
                bump("cut_axis%d_side%d" % (axis, side))
                if append(m2, L[idx]["kind"], L[idx]["src"], L[idx]["members"], 2):
                    L[idx]["plane"], L[idx]["split"] = m1, 1
                    rep["splits"] += 1
                break
        else:
            bump("exhausted_splits")
    # 6. delete
    kept = [e for idx, e in enumerate(L) if not d["delete_act"][idx]]
    rep["deleted"] = len(L) - len(kept)
    rep["count"] = len(kept)
    masks, info = np.zeros((M, h, w), np.uint8), np.zeros((M, 4), np.int32)
    for o, e in enumerate(kept):
        masks[o] = e["plane"].astype(np.uint8) * 255
        info[o] = (e["kind"], e["src"], e["members"], e["split"])
    return masks, info, np.array([rep[k] for k in REPORT], np.int32)


def scene_perturb_batch_np(gt, props, n_gt, n_prop, M, min_mask_ratio, draws):
    """gt u8 [B,N,h,w], props u8 [B,P,h,w], n_gt / n_prop [B], draws: ScenePerturb.draws()'s stacked tables ->
    (masks u8 [B,M,h,w], info i32 [B,M,4], report i32 [B,8])."""
    out = [scene_perturb_np(gt[b], props[b], int(n_gt[b]), int(n_prop[b]), M, min_mask_ratio, {k: v[b] for k, v in draws.items()})
           for b in range(len(gt))]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


# ---- the reference's stage in its own dtypes ----
def compute_iou_u8(seg, gt):
    """perturbation_utils.py:34-37 on uint8 arrays: products and sums wrap."""
    return (np.count_nonzero(seg * gt) + 1e-6) / (np.count_nonzero(seg + gt) + 1e-6)


def dilate10_u8(m):
    """cv2.dilate(m, np.ones((10, 10), np.uint8)) as OpenCV documents it (the module docstring): a max over the 10 x 10 window anchored
    at (5, 5), 0 beyond the frame."""
    h, w = m.shape
    p = np.zeros((h + 10, w + 10), np.uint8)
    p[5:5 + h, 5:5 + w] = m
    out = np.zeros((h, w), np.uint8)
    for i in range(10):
        for j in range(10):
            out = np.maximum(out, p[i:i + h, j:j + w])
    return out


def reference_scene(gt01, props01, min_mask_ratio, d):
    """perturbate_masks.py:101-205 for one frame: gt01 / props01 uint8 0 / 1 [n,h,w]; every coin the script flips is read from the
    tables d (``random.random() > ratio: continue`` = not act; the split's randint / coins = split_try) -> list of uint8 [h,w]."""
    h, w = gt01.shape[1:] if len(gt01) else props01.shape[1:]
    lim = w * h * min_mask_ratio
    out = []
    max_area = np.max([np.sum(g) for g in gt01]) if len(gt01) else 0      # (np.max of an empty list raises in the script)
    for q, p in enumerate(props01):
        if not d["fp_act"][q]:
            continue
        if np.sum(p) < lim or np.sum(p) > max_area * 2.0:
            continue
        best = 0
        for g in gt01:
            best = max(best, compute_iou_u8(g, p))
        if best < 0.3:
            out.append(p * np.uint8(255))
    for q, p in enumerate(props01):
        if not d["gs_act"][q]:
            continue
        if np.sum(p) < lim:
            continue
        best = 0
        for g in gt01:
            best = max(best, compute_iou_u8(g, p))
        if best > 0.3:
            out.append(p * np.uint8(255))
    unused = []
    for g in gt01:
        best = 0
        for m in out:
            best = max(best, compute_iou_u8(g, m))       # 0 / 1 plus 0 / 255 in uint8
        if best < 0.3:
            unused.append(g * np.uint8(255))
    out.extend(unused)
    for i1 in range(len(out)):
        if not d["merge_act"][i1]:
            continue
        first = out[i1]
        for i2 in range(len(out)):
            if i1 == i2:
                continue
            second = out[i2]
            if np.sum(dilate10_u8(first.copy()) * second) > 0:
                out[i1] = first + second
                out[i2] = np.zeros_like(second)
    out = [m for m in out if np.sum(m) > 0]
    for i in range(len(out)):
        if not d["split_act"][i]:
            continue
        ok = False
        for k in range(ATTEMPTS):
            m = out[i]
            ys, xs = np.where(m != 1)
            x_min, y_min, x_max, y_max = np.min(xs), np.min(ys), np.max(xs), np.max(ys)
            assert (x_min, y_min, x_max, y_max) == (0, 0, w - 1, h - 1)      # the box of `mask != 1` on a 0 / 255 mask is the frame
            x1, y1, axis, side = (int(v) for v in d["split_try"][i][k])       # randint(x_min, x_max), randint(y_min, y_max), two coins
            a = m.copy()
            if axis == 0:
                if side == 0:
                    a[y1:y_max, :] = 0
                else:
                    a[y_min:y1, :] = 0
            else:
                if side == 0:
                    a[:, x1:x_max] = 0
                else:
                    a[:, x_min:x1] = 0
            b = np.where(a != 0, 0, m.copy())
            if np.sum(a) < lim or np.sum(b) < lim:
                continue
            ok = True
            break
        if ok:
            out[i] = a
            out.append(b)
    return [m for i, m in enumerate(out) if not d["delete_act"][i]]


# ---- scenes ----
def ellipse(h, w, cy, cx, ry, rx):
    y, x = np.mgrid[:h, :w]
    return ((y - cy) / max(ry, 0.5)) ** 2 + ((x - cx) / max(rx, 0.5)) ** 2 <= 1.0


def random_ellipse(rng, h, w):
    return ellipse(h, w, rng.uniform(0, h), rng.uniform(0, w), rng.uniform(2, h / 2.5), rng.uniform(2, w / 2.5))


ACT = (0.6, 0.6, 0.4, 0.6, 0.2)        # fp, gs, merge, split, delete
MIN_RATIO = 0.05


def random_scene(seed, shape=None, n=None, p=None):
    """A frame of 20-50 x 20-70 (or `shape`) with 1-6 ellipses as ground truth (or n) and 0-6 proposals (or p) that are fresh ellipses,
    truncated ground truths or ground truths grown by an ellipse; the tables drawn with the act probabilities ACT and M = 2 (N + P) + 4.
    -> dict(gt u8 0 / 1 [n,h,w], props u8 0 / 1 [p,h,w], M, d)."""
    rng = np.random.RandomState(seed)
    h, w = shape if shape is not None else (rng.randint(20, 51), rng.randint(20, 71))
    n = rng.randint(1, 7) if n is None else n
    p = rng.randint(0, 7) if p is None else p
    gt = np.zeros((n, h, w), np.uint8)
    for g in range(n):
        gt[g] = random_ellipse(rng, h, w)
    props = np.zeros((p, h, w), np.uint8)
    for q in range(p):
        how = rng.randint(3) if n else 0
        if how == 0:
            props[q] = random_ellipse(rng, h, w)
        elif how == 1:
            props[q] = gt[rng.randint(n)] & cut_region(h, w, rng.randint(w), rng.randint(h), rng.randint(2), rng.randint(2))
        else:
            props[q] = gt[rng.randint(n)] | random_ellipse(rng, h, w)
    M = 2 * (n + p) + 4
    return {"gt": gt, "props": props, "M": M, "d": scene_draws(rng, p, M, h, w, *ACT)}


N_SEEDS = 300


def test_contract_equals_the_reference_description_on_random_scenes():
    stats, tot = {}, dict.fromkeys(REPORT, 0)
    for seed in range(N_SEEDS):
        s = random_scene(seed)
        n, p = len(s["gt"]), len(s["props"])
        masks, info, rep = scene_perturb_np(s["gt"], s["props"], n, p, s["M"], MIN_RATIO, s["d"], stats)
        want = reference_scene(s["gt"], s["props"], MIN_RATIO, s["d"])
        assert rep[0] == len(want), seed
        assert rep[7] == 0, seed                                           # M = 2 (N + P) + 4 never drops
        for o, m in enumerate(want):
            assert np.array_equal(masks[o] != 0, m != 0), (seed, o)
        assert not masks[rep[0]:].any() and not info[rep[0]:].any()
        assert set(np.unique(masks)) <= {0, 255}
        for k, v in zip(REPORT, rep):
            tot[k] += int(v)
    # the agreement is not vacuous: every branch is reached
    assert tot["n_fp"] > 0 and tot["n_gs"] > 0 and tot["gt_kept"] > 0 and tot["absorbed"] > 0 and tot["splits"] > 0 and tot["deleted"] > 0
    for key in ("gt_replaced", "multi_absorption_merges", "exhausted_splits", "wrapped_union_decides", "absorbed_before_own_turn",
                "cut_axis0_side0", "cut_axis0_side1", "cut_axis1_side0", "cut_axis1_side1"):
        assert stats.get(key, 0) > 0, (key, stats)


# ---- hand-drawn cases ----
def quiet(P, M):
    """Tables in which nothing acts."""
    z = lambda *s: np.zeros(s, np.uint8)
    return {"fp_act": z(P), "gs_act": z(P), "merge_act": z(M), "split_act": z(M), "delete_act": z(M),
            "split_try": np.zeros((M, ATTEMPTS, 4), np.int32)}


def boxes(h, w, *rects):
    """u8 [n,h,w]: one 0 / 1 rectangle (y0, y1, x0, x1), ends exclusive, per plane."""
    out = np.zeros((len(rects), h, w), np.uint8)
    for i, (y0, y1, x0, x1) in enumerate(rects):
        out[i, y0:y1, x0:x1] = 1
    return out


_RECORD = None          # hand_cases(): the list that receives the inputs of every run() below


def run(gt, props, M, d, ratio=0.0):
    gt = np.asarray(gt, np.uint8)
    props = np.zeros((0,) + gt.shape[1:], np.uint8) if props is None else np.asarray(props, np.uint8)
    if _RECORD is not None:
        _RECORD.append((gt.copy(), props.copy(), M, {k: np.array(v) for k, v in d.items()}, ratio))
    masks, info, rep = scene_perturb_np(gt, props, len(gt), len(props), M, ratio, d)
    return masks, info, dict(zip(REPORT, (int(v) for v in rep)))


def hand_cases():
    """Every frame the hand-drawn tests below put through the contract, as (gt, props, M, tables, min_mask_ratio): the GPU tests replay
    them on the device."""
    global _RECORD
    _RECORD = out = []
    try:
        for fn in (test_dilation_anchor_is_asymmetric, test_merge_keeps_only_the_last_of_several_touching_masks,
                   test_mask_absorbed_before_its_own_turn_does_nothing, test_tie_of_three_tenths_is_an_over_segmentation_not_a_false_positive,
                   test_the_wrapped_union_decides_step_3, test_false_positive_area_filter, test_the_four_cuts_and_the_last_row_and_column,
                   test_a_line_on_the_last_row_cuts_nothing_and_the_next_attempt_is_taken, test_no_ground_truth_no_proposals_and_an_empty_mask,
                   test_capacity_in_step_3_and_in_step_5, test_delete_and_order):
            fn()
    finally:
        _RECORD = None
    return out


def test_dilation_anchor_is_asymmetric():
    # a at columns 20..21; a partner whose first column is 5 to the right of a's last one is touched, 6 is not; to the left 4 is, 5 is not
    for dist, right, left in ((4, True, True), (5, True, False), (6, False, False)):
        h, w = 12, 48
        for where, want in (("right", right), ("left", left)):
            x = 21 + dist if where == "right" else 20 - dist
            gt = boxes(h, w, (4, 6, 20, 22), (4, 6, x, x + 1))
            d = quiet(0, 4)
            d["merge_act"][0] = 1
            _, info, rep = run(gt, None, 4, d)
            assert (rep["absorbed"] == 1) == want and rep["count"] == (1 if want else 2), (dist, where)
            # and likewise for rows
            gt = boxes(w, h, (20, 22, 4, 6), (x, x + 1, 4, 6))
            _, info, rep = run(gt, None, 4, d)
            assert (rep["absorbed"] == 1) == want, (dist, where, "rows")
    # the dilation belongs to the mask whose turn it is: with the turn on the RIGHT mask, a distance of 5 does not merge
    gt = boxes(12, 48, (4, 6, 20, 22), (4, 6, 26, 27))
    d = quiet(0, 4)
    d["merge_act"][1] = 1
    assert run(gt, None, 4, d)[2]["absorbed"] == 0


def test_merge_keeps_only_the_last_of_several_touching_masks():
    gt = boxes(10, 60, (2, 5, 20, 24), (2, 5, 10, 18), (2, 5, 26, 30))      # 0 touches both 1 (to its left) and 2 (to its right)
    d = quiet(0, 6)
    d["merge_act"][0] = 1
    masks, info, rep = run(gt, None, 6, d)
    assert rep["count"] == 1 and rep["absorbed"] == 2
    assert np.array_equal(masks[0] != 0, (gt[0] | gt[2]) != 0)               # mask 1 is lost: absorbed, then overwritten
    assert tuple(info[0]) == (0, 0, 2, 0)


def test_mask_absorbed_before_its_own_turn_does_nothing():
    gt = boxes(10, 60, (2, 5, 10, 14), (2, 5, 16, 20), (2, 5, 22, 26))
    d = quiet(0, 6)
    d["merge_act"][0] = d["merge_act"][1] = 1
    masks, info, rep = run(gt, None, 6, d)
    # turn 0 absorbs 1 (2 is out of reach of mask 0 alone); at turn 1 slot 1 is empty, so 2 stays on its own
    assert rep["count"] == 2 and rep["absorbed"] == 1
    assert np.array_equal(masks[0] != 0, (gt[0] | gt[1]) != 0) and np.array_equal(masks[1] != 0, gt[2] != 0)
    assert tuple(info[0]) == (0, 0, 2, 0) and tuple(info[1]) == (0, 2, 1, 0)
    # a later turn sees the members gathered so far: 2 then 0 - slot 0 = {0, 1} reaches 2 through member 1
    d = quiet(0, 6)
    d["merge_act"][0] = 1
    gt2 = gt[[0, 2, 1]]                                                     # slot 1 is now the far mask, slot 2 the middle one
    d["merge_act"][2] = 1
    masks, info, rep = run(gt2, None, 6, d)
    # turn 0: A = {0}, touches slot 2 (the middle) -> {0, 2}; turn 2: empty, nothing
    assert rep["count"] == 2 and rep["absorbed"] == 1


def test_tie_of_three_tenths_is_an_over_segmentation_not_a_false_positive():
    h, w = 4, 16
    gt = boxes(h, w, (0, 1, 0, 7))                  # 7 pixels
    props = boxes(h, w, (0, 1, 4, 10))              # 6 pixels, 3 shared: 3 / 10
    assert (3 + 1e-6) / (10 + 1e-6) > 0.3
    d = quiet(1, 6)
    d["fp_act"][0] = d["gs_act"][0] = 1
    masks, info, rep = run(gt, props, 6, d)
    assert (rep["n_fp"], rep["n_gs"]) == (0, 1) and tuple(info[0]) == (2, 0, 1, 0)
    # step 3 of the same frame: 3 / (10 - 3) >= 0.3, the ground truth counts as covered
    assert rep["gt_kept"] == 0 and rep["count"] == 1


def test_the_wrapped_union_decides_step_3():
    h, w = 4, 40
    gt = boxes(h, w, (0, 1, 0, 10))                 # 10 pixels
    props = boxes(h, w, (0, 1, 6, 30))              # 24 pixels, 4 shared: the IoU is 4 / 30 < 0.3, fp; 4 / (30 - 4) < 0.3 too
    d = quiet(1, 6)
    d["fp_act"][0] = 1
    assert run(gt, props, 6, d)[2]["gt_kept"] == 1
    props = boxes(h, w, (0, 1, 5, 18))              # 13 pixels, 5 shared: 5 / 18 < 0.3 -> fp, but 5 / (18 - 5) > 0.3 -> covered
    _, info, rep = run(gt, props, 6, d)
    assert (rep["n_fp"], rep["gt_kept"], rep["count"]) == (1, 0, 1)


def test_false_positive_area_filter():
    h, w = 10, 20                                   # lim = 200 * 0.05 = 10
    gt = boxes(h, w, (0, 3, 0, 4))                  # 12 pixels: proposals above 24 are too large
    props = boxes(h, w, (5, 8, 10, 13), (5, 10, 10, 15), (5, 8, 10, 18), (5, 7, 10, 15))     # 9 (small), 25 (large), 24, 10
    d = quiet(4, 12)
    d["fp_act"][:] = 1
    _, info, rep = run(gt, props, 12, d, ratio=0.05)
    assert rep["n_fp"] == 2 and [tuple(r) for r in info[:2]] == [(1, 2, 1, 0), (1, 3, 1, 0)]


def test_the_four_cuts_and_the_last_row_and_column():
    h, w = 8, 9
    gt = np.ones((1, h, w), np.uint8)
    for (axis, side, x1, y1), (want2,) in (((0, 0, 3, 2), (np.s_[2:h - 1, :],)), ((0, 1, 3, 2), (np.s_[:2, :],)),
                                           ((1, 0, 3, 2), (np.s_[:, 3:w - 1],)), ((1, 1, 3, 2), (np.s_[:, :3],))):
        d = quiet(0, 4)
        d["split_act"][0] = 1
        d["split_try"][0, :] = (x1, y1, axis, side)
        masks, info, rep = run(gt, None, 4, d)
        cut = np.zeros((h, w), bool)
        cut[want2] = True
        assert rep["splits"] == 1 and rep["count"] == 2
        assert np.array_equal(masks[1] != 0, cut) and np.array_equal(masks[0] != 0, ~cut)
        assert tuple(info[0]) == (0, 0, 1, 1) and tuple(info[1]) == (0, 0, 1, 2)
        if side == 0:                                # the last row / column survives in the kept half
            assert masks[0][h - 1].all() if axis == 0 else masks[0][:, w - 1].all()


def test_a_line_on_the_last_row_cuts_nothing_and_the_next_attempt_is_taken():
    h, w = 8, 9
    gt = np.ones((1, h, w), np.uint8)
    d = quiet(0, 4)
    d["split_act"][0] = 1
    d["split_try"][0, :] = (0, h - 1, 0, 0)          # y1 >= h - 1: rows [h - 1, h - 1) are empty, mask2 is empty, invalid at lim > 0
    masks, info, rep = run(gt, None, 4, d, ratio=0.05)
    assert rep["splits"] == 0 and rep["count"] == 1 and info[0][3] == 0
    d["split_try"][0, 7] = (0, 4, 0, 1)              # the first valid attempt wins
    d["split_try"][0, 8] = (0, 2, 0, 1)
    masks, info, rep = run(gt, None, 4, d, ratio=0.05)
    assert rep["splits"] == 1 and np.count_nonzero(masks[1]) == 4 * w
    # halves are compared as 255 x pixels (the reference sums bytes): ONE pixel passes a limit of 72, the whole frame's area
    d["split_try"][0, :] = (1, 0, 1, 1)              # columns [0, 1) of a single-row mask: 1 pixel against 8
    one = boxes(h, w, (0, 1, 0, 9))
    masks, info, rep = run(one, None, 4, d, ratio=1.0)
    assert rep["splits"] == 1 and np.count_nonzero(masks[1]) == 1 and np.count_nonzero(masks[0]) == 8


def test_no_ground_truth_no_proposals_and_an_empty_mask():
    h, w = 10, 20
    props = boxes(h, w, (0, 5, 0, 5))
    d = quiet(1, 4)
    d["fp_act"][0] = d["gs_act"][0] = 1
    # n_gt = 0: the largest ground truth is 0, every non-empty proposal is too large, none can be an over-segmentation
    _, _, rep = run(np.zeros((0, h, w), np.uint8), props, 4, d)
    assert rep == dict.fromkeys(REPORT, 0)
    # n_prop = 0: the ground truth passes through
    gt = boxes(h, w, (0, 5, 0, 5), (6, 9, 10, 15))
    masks, info, rep = run(gt, None, 4, quiet(0, 4))
    assert rep["count"] == 2 and rep["gt_kept"] == 2 and np.array_equal(masks[:2], gt * 255)
    # an all-empty ground truth is appended by step 3 and removed with the empty entries after the merge
    gt = np.concatenate([boxes(h, w, (0, 5, 0, 5)), np.zeros((1, h, w), np.uint8), boxes(h, w, (6, 9, 10, 15))])
    masks, info, rep = run(gt, None, 4, quiet(0, 4))
    assert rep["count"] == 2 and rep["gt_kept"] == 3 and [int(r[1]) for r in info[:2]] == [0, 2]


def test_capacity_in_step_3_and_in_step_5():
    h, w = 10, 40
    gt = boxes(h, w, (0, 4, 0, 4), (0, 4, 20, 24), (6, 9, 0, 4))
    masks, info, rep = run(gt, None, 2, quiet(0, 2))
    assert (rep["count"], rep["gt_kept"], rep["dropped"]) == (2, 2, 1)
    d = quiet(0, 3)
    d["split_act"][:] = 1
    d["split_try"][:, :] = (2, 2, 0, 1)              # rows [0, 2)
    masks, info, rep = run(gt[:2], None, 3, d)
    # the first split takes the last free slot, the second is not performed as a whole
    assert (rep["count"], rep["splits"], rep["dropped"]) == (3, 1, 1)
    assert [int(r[3]) for r in info[:3]] == [1, 0, 2] and np.array_equal(masks[1] != 0, gt[1] != 0)


def test_delete_and_order():
    h, w = 10, 40
    gt = boxes(h, w, (0, 4, 0, 4), (0, 4, 20, 24), (6, 9, 30, 34))
    d = quiet(0, 6)
    d["delete_act"][1] = 1
    masks, info, rep = run(gt, None, 6, d)
    assert (rep["count"], rep["deleted"]) == (2, 1) and [int(r[1]) for r in info[:2]] == [0, 2]
    assert not masks[2:].any() and not info[2:].any()


# ---- the host-side API ----
def test_scene_draws_order():
    P, M, h, w = 3, 5, 17, 23
    d = scene_draws(np.random.RandomState(11), P, M, h, w)
    r = np.random.RandomState(11)
    ratios = [r.uniform(*DEFAULT_RANGES[k]) for k in ("fp", "gs", "merge", "split", "delete")]
    assert np.array_equal(d["ratios"], ratios)
    assert np.array_equal(d["fp_act"], r.random_sample(P) <= ratios[0])
    assert np.array_equal(d["gs_act"], r.random_sample(P) <= ratios[1])
    assert np.array_equal(d["merge_act"], r.random_sample(M) <= ratios[2])
    assert np.array_equal(d["split_act"], r.random_sample(M) <= ratios[3])
    for k in range(M):
        for a in range(ATTEMPTS):
            x1 = r.randint(w)
            y1 = r.randint(h)
            axis = 0 if r.random_sample() < 0.5 else 1
            side = 0 if r.random_sample() < 0.5 else 1
            assert tuple(d["split_try"][k, a]) == (x1, y1, axis, side)
    assert np.array_equal(d["delete_act"], r.random_sample(M) <= ratios[4])
    assert np.array_equal(d["walk_targets"], r.uniform(0.8, 1.0, M))
    assert d["split_try"].dtype == np.int32 and d["fp_act"].dtype == np.uint8 and d["walk_targets"].dtype == np.float64
    assert d["split_try"][..., 0].max() < w and d["split_try"][..., 1].max() < h
    # a plain number is taken as it stands and draws nothing
    d = scene_draws(np.random.RandomState(11), P, M, h, w, 1.0, 0.0, 0.5, (0.25, 0.25), 1)
    r = np.random.RandomState(11)
    assert r.uniform(0.25, 0.25) == 0.25 and list(d["ratios"]) == [1.0, 0.0, 0.5, 0.25, 1.0]
    assert d["fp_act"].all() and np.array_equal(d["fp_act"], r.random_sample(P) <= 1.0) and not d["gs_act"].any()


def test_scene_perturb_options():
    s = ScenePerturb(seed=5, max_masks=7)
    assert s.min_mask_ratio == 0.01 and s.ratios == tuple(DEFAULT_RANGES[k] for k in ("fp", "gs", "merge", "split", "delete"))
    d = s.draws(2, 3, 17, 23)
    for b in range(2):
        one = scene_draws(np.random.RandomState(5 + b), 3, 7, 17, 23)
        assert all(np.array_equal(d[k][b], one[k]) for k in one)
    assert d is s.draws(2, 3, 17, 23) and not d["fp_act"].flags.writeable
    assert s.walk_targets(2).shape == (2, 7) and np.array_equal(s.walk_targets(2), d["walk_targets"])
    assert np.array_equal(s.walk_targets(2, 3, 17, 23), d["walk_targets"])
    with pytest.raises(ValueError):
        ScenePerturb().walk_targets(2)               # nothing has fixed n_prop, h, w yet
    assert ScenePerturb(seed=5, max_masks=7) == s and hash(ScenePerturb(seed=5, max_masks=7)) == hash(s) and ScenePerturb(seed=6, max_masks=7) != s
    assert ScenePerturb.parse(None) is None and ScenePerturb.parse(s) is s
    assert "max_masks=7" in repr(s)
    for bad in (dict(seed=-1), dict(seed=1.0), dict(seed=True), dict(max_masks=0), dict(max_masks=MAX_SLOTS + 1), dict(max_masks=2.0),
                dict(min_mask_ratio=-0.1), dict(min_mask_ratio=1.5), dict(min_mask_ratio=float("nan")), dict(min_mask_ratio="x"),
                dict(fp=1.5), dict(gs=(0.5, 0.2)), dict(merge=(0.1, 0.2, 0.3)), dict(split=True), dict(delete=(0.0, 2.0))):
        with pytest.raises(ValueError):
            ScenePerturb(**bad)
    with pytest.raises(ValueError):
        ScenePerturb.parse("largest")
    # the predictor's options: off by default, refused together with what has no scene form
    from quber_amd.maskrefiner.predictor import RefineOptions
    from quber_amd.meanshift import MeanShift
    from quber_amd.zoom import ZoomIn
    assert RefineOptions.parse().scene is None and RefineOptions.parse(scene=s, nms=None).scene is s
    for bad in (dict(scene="x"), dict(scene=s, zoom=ZoomIn()), dict(scene=s, cluster=MeanShift())):
        with pytest.raises(ValueError, match="scene"):
            RefineOptions.parse(**bad)


def test_abi_entry_is_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "quber_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+quber_scene_perturb\s*\(", code)
    assert "quber_scene_perturb" in _lib.SIGNATURES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "quber_scene_perturb")
    n_args = len([a for a in re.search(r"quber_scene_perturb\s*\((.*?)\)", code, flags=re.S).group(1).split(",") if a.strip()])
    assert n_args == len(_lib.SIGNATURES["quber_scene_perturb"][1])


# ---- the scenes the GPU tests run (tests/test_gpu_scene.py) ----
GPU_FRAMES = ((24, 40), (33, 64), (37, 70), (20, 131))
# (N, P, M): every N, P in {0, 1, 5, 17} with every other, M = 16 where the list can fit it and 40 elsewhere, (1, 1) and (5, 5) with both
GPU_COUNTS = tuple((N, P, 16 if N + P <= 10 else 40) for N in (0, 1, 5, 17) for P in (0, 1, 5, 17)) + ((1, 1, 40), (5, 5, 40))
_GPU_BATCHES = {}


def gpu_batch(shape, N, P, M, ratio=MIN_RATIO):
    """A batch of 3 frames at `shape` with N / P mask rows and different n_gt / n_prop per frame (frame 0 uses all rows) -> dict of
    gt u8 [3,N,h,w], props u8 [3,P,h,w] (0 / 1, rows behind the counts zero), n_gt, n_prop i32 [3], the stacked tables at capacity M and
    the contract's outputs.  The scenes are chosen here, on the CPU: the first seed for which the contract drops nothing, so that a
    device that drops masks cannot hide behind the capacity rule.  Computed once per process."""
    key = (shape, N, P, M, ratio)
    if key in _GPU_BATCHES:
        return _GPU_BATCHES[key]
    h, w = shape
    B = 3
    n_gt = np.array([N, N // 2, max(N - 1, 0)], np.int32)
    n_prop = np.array([P, max(P - 1, 0), P // 3], np.int32)
    for seed in range(64):
        gt, props = np.zeros((B, N, h, w), np.uint8), np.zeros((B, P, h, w), np.uint8)
        per = []
        for b in range(B):
            base = 100003 * seed + 1009 * (N * 31 + P) + 17 * h + w + b
            s = random_scene(base, shape, int(n_gt[b]), int(n_prop[b]))
            gt[b, :n_gt[b]], props[b, :n_prop[b]] = s["gt"], s["props"]
            per.append(scene_draws(np.random.RandomState(base + 7), P, M, h, w, *ACT))
        draws = {k: np.ascontiguousarray(np.stack([p[k] for p in per])) for k in per[0]}
        want = scene_perturb_batch_np(gt, props, n_gt, n_prop, M, ratio, draws)
        if not want[2][:, 7].any():
            break
    else:
        raise AssertionError(f"no seed without a dropped mask for {key}")
    out = {"gt": gt, "props": props, "n_gt": n_gt, "n_prop": n_prop, "draws": draws, "M": M, "ratio": ratio, "want": want}
    _GPU_BATCHES[key] = out
    return out


def test_gpu_scenes_never_drop_and_reach_every_stage():
    """The condition on the GPU tests' inputs: for every scene but the capacity cases the contract alone reports dropped = 0."""
    seen = dict.fromkeys(REPORT, 0)
    for shape in GPU_FRAMES:
        for N, P, M in GPU_COUNTS:
            rep = gpu_batch(shape, N, P, M)["want"][2]
            assert not rep[:, 7].any(), (shape, N, P, M)
            for k, v in zip(REPORT, rep.sum(0)):
                seen[k] += int(v)
    assert all(seen[k] > 0 for k in REPORT if k != "dropped"), seen
