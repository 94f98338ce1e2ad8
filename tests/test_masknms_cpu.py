"""CPU: the contract of the mask NMS that makes scored, overlapping initial masks disjoint (csrc/masknms.hip, Engine.mask_nms,
MaskRefinerPredictor(nms=MaskNMS())), stated in numpy, and what can be checked of the feature without a GPU.

The reference runs the same three loops in three places (eval/refiner_model.py:683-740, eval/base_model.py:1027-1086 and 1154-1190):
``nms`` - all pairwise intersections by ``np.sum(np.multiply(masks[i], masks[j]))`` into a float32 table, a greedy pass in score order
that keeps a mask and drops every later one whose IoU with it exceeds 0.7, the survivors ordered by area - and
``combine_masks_with_NMS``, which paints the survivors one after the other into one label map (labels from 2, a later one overwrites);
its callers then take ``masks == id`` for ``np.unique(masks)[1:]``.  ``reference_nms_combine`` below is a literal transcription of these
loops; ``mask_nms_np`` is the contract in this repository's words, and the device is held to it bit for bit (tests/test_gpu_masknms.py).

Where the contract pins what the reference leaves open:
  * the reference's ``scores.argsort()`` and ``np.argsort(areas[keep])`` use numpy's default sort, which leaves the order of equal keys
    to the numpy build.  The contract: ``kind="stable"`` in both - among equal scores the HIGHER index is visited first (the stable
    ascending order reversed), among survivors of equal area the one visited earlier is painted first.  The comparison with the
    transcription therefore uses proposal sets with distinct scores and distinct areas, where the reference is deterministic.
  * ``ovr`` is evaluated in float32 in exactly the reference's order, ``inter / ((area_i + area_j) - inter)``, and compared with
    ``float32(thresh)`` (what numpy does with a float32 array and a Python float).  H * W <= 2^24, so every count is exact in float32.
  * a mask whose score is NaN is absent: never visited, kept or painted.  (The reference has no such thing; it is how a frame with
    fewer masks than the batch's N is padded on the device.)
Stated, not tested:
  * ``np.multiply`` of two uint8 masks of 255 wraps to 1 (255 * 255 = 65025 = 254 * 256 + 1), and of two bools or 0 / 1 masks it is 1
    as well: the reference's count is the number of pixels inside both for bool and for 0 / 255 inputs alike.  The contract counts
    non-zero pixels.
  * the reference's ``score_mask`` and ``bbox`` by-products are not reproduced (its ``np.min`` of an empty survivor's coordinates even
    raises; here an empty survivor is simply never visible).
"""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from quber_amd import _lib
from quber_amd.masknms import MAX_MASKS, MaskNMS, check_scores


# ---- the contract ----
def mask_nms_np(masks, scores, thresh=0.7, on_top="large"):
    """One frame.  masks [N,H,W] (non-zero = inside), scores float32 [N] (finite; NaN = no such mask), H * W <= 2^24 ->
    (out u8 [N,H,W] of 0 / 255: the disjoint masks, compacted to the front, zero planes behind; count; source i32 [N]: the input index of
    each output mask, -1 behind count; kept: the survivors of the NMS, before hidden ones drop out; ids i32 [H,W]: 0, 1..count;
    out_scores f32 [N]: the output masks' scores, 0 behind count)."""
    m = np.asarray(masks) != 0
    n, h, w = m.shape
    assert h * w <= 2 ** 24 and on_top in ("large", "small")
    scores = np.asarray(scores, np.float32)
    assert scores.shape == (n,)
    flat = m.reshape(n, h * w).astype(np.float32)
    inter = flat @ flat.T                # refiner_model.py:686-690: pixels inside both, as float32 (exact: every partial sum is an integer <= 2^24)
    area = np.diag(inter).copy()                                 # :692
    present = np.flatnonzero(~np.isnan(scores))
    order = present[np.argsort(scores[present], kind="stable")[::-1]]      # :693, ties: the higher index first
    t = np.float32(thresh)
    alive = np.ones(len(order), bool)
    keep = []
    for p, i in enumerate(order):                                # :695-701
        if not alive[p]:
            continue
        keep.append(i)
        for q in range(p + 1, len(order)):
            if alive[q]:
                j = order[q]
                with np.errstate(invalid="ignore", divide="ignore"):
                    ovr = inter[i, j] / ((area[i] + area[j]) - inter[i, j])        # float32 throughout
                alive[q] = bool(ovr <= t)                        # a NaN (two empty masks) suppresses
    keep = np.array(keep, np.int64)
    paint = keep[np.argsort(area[keep], kind="stable")] if len(keep) else keep      # :703-704
    if on_top == "small":
        paint = paint[::-1]
    painted = np.zeros((h, w), np.int32)
    for k, i in enumerate(paint):                                # :728-730, a later one overwrites (labels from 1 here)
        painted[m[i]] = k + 1
    visible = np.unique(painted)
    visible = visible[visible > 0]
    out = np.zeros((n, h, w), np.uint8)
    source = np.full((n,), -1, np.int32)
    out_scores = np.zeros((n,), np.float32)
    ids = np.zeros((h, w), np.int32)
    for k, v in enumerate(visible):
        out[k][painted == v] = 255
        ids[painted == v] = k + 1
        source[k] = paint[v - 1]
        out_scores[k] = scores[paint[v - 1]]
    return out, len(visible), source, len(keep), ids, out_scores


def mask_nms_batch_np(masks, scores, thresh=0.7, on_top="large"):
    """[B,N,H,W], [B,N] -> (out [B,N,H,W], ids [B,H,W], source [B,N], out_scores [B,N], report i32 [B,4]: count, kept, 0, 0)."""
    res = [mask_nms_np(m, s, thresh, on_top) for m, s in zip(masks, scores)]
    report = np.array([[r[1], r[3], 0, 0] for r in res], np.int32).reshape(len(res), 4)
    return (np.stack([r[0] for r in res]), np.stack([r[4] for r in res]), np.stack([r[2] for r in res]),
            np.stack([r[5] for r in res]), report)


# ---- the reference's loops, transcribed (eval/refiner_model.py:683-704 and 714-730; base_model.py:1065-1086 and 1037-1053 are the same) ----
def reference_nms_combine(mask, scores, thresh=0.7):
    """-> the list of masks ``bin_mask == id`` for ``np.unique(bin_mask)[1:]`` and the input index of each."""
    masks = mask
    n = masks.shape[0]
    inters = np.zeros((n, n), dtype=np.float32)
    for i in range(n):
        for j in range(i, n):
            inters[i, j] = np.sum(np.multiply(masks[i], masks[j]))
            inters[j, i] = inters[i, j]
    areas = np.diag(inters)
    order = scores.argsort()[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(i)
        inter = inters[i, order[1:]]
        with np.errstate(invalid="ignore", divide="ignore"):
            ovr = inter / (areas[i] + areas[order[1:]] - inter)
        inds = np.where(ovr <= thresh)[0]
        order = order[inds + 1]
    index = np.argsort(areas[keep]).astype(np.int32)
    keep = np.array(keep)[index].astype(int)
    mask = mask[keep]
    num, h, w = mask.shape
    bin_mask = np.zeros((h, w))
    for m, object_label in zip(mask, range(2, 2 + len(mask))):
        label_pos = np.nonzero(m)
        bin_mask[label_pos] = object_label
    labels = np.unique(bin_mask)[1:]
    return [bin_mask == v for v in labels], [int(keep[int(v) - 2]) for v in labels]


# ---- proposal sets (shared with the GPU tests) ----
def blob(h, w, cy, cx, ry, rx):
    y, x = np.mgrid[:h, :w]
    return ((y - cy) / max(ry, 0.5)) ** 2 + ((x - cx) / max(rx, 0.5)) ** 2 <= 1.0


def proposals(h, w, n, seed, distinct=True, value=255):
    """n scored proposals of a few objects: overlapping blobs, near and exact duplicates, nested ones.  distinct: the scores are distinct,
    and the masks are nudged until their areas are (the case in which the reference is deterministic) -> (masks u8 [n,h,w], f32 [n])."""
    rng = np.random.RandomState(seed)
    n_obj = max(1, n // 3)
    objs = [(rng.uniform(0.15, 0.85) * h, rng.uniform(0.15, 0.85) * w, rng.uniform(0.1, 0.3) * h, rng.uniform(0.1, 0.3) * w) for _ in range(n_obj)]
    masks = np.zeros((n, h, w), bool)
    for i in range(n):
        cy, cx, ry, rx = objs[rng.randint(n_obj)]
        kind = rng.randint(4) if i else 0
        if kind == 1 and i:                                      # an exact duplicate of an earlier proposal
            masks[i] = masks[rng.randint(i)]
            continue
        if kind == 2:                                            # a part nested inside the object
            ry, rx, cy = ry * 0.45, rx * 0.45, cy + 0.2 * ry
        elif kind == 3:                                          # a near duplicate: jittered
            cy, cx, ry, rx = cy + rng.uniform(-1.5, 1.5), cx + rng.uniform(-1.5, 1.5), ry * rng.uniform(0.9, 1.1), rx * rng.uniform(0.9, 1.1)
        masks[i] = blob(h, w, cy, cx, ry, rx)
    if distinct:
        seen = set()
        for i in range(n):
            free = np.flatnonzero(~masks[i].ravel())
            k = 0
            while int(masks[i].sum()) in seen or not masks[i].any():       # one more pixel until the area is new
                masks[i].ravel()[free[k]] = True
                k += 1
            seen.add(int(masks[i].sum()))
        scores = (rng.permutation(n) + 1).astype(np.float32) / np.float32(n + 1)
    else:
        scores = rng.randint(1, 4, n).astype(np.float32) / np.float32(4)
    return masks.astype(np.uint8) * np.uint8(value), scores


SEEDED = [(24, 40, n, s) for s, n in enumerate([1, 2, 3, 5, 8, 13, 21, 40, 7, 11, 30])] + \
         [(70, 131, n, 20 + s) for s, n in enumerate([1, 2, 4, 6, 9, 15, 16, 17, 25, 33, 40])]


@pytest.mark.parametrize("h,w,n,seed", SEEDED, ids=["%dx%d-n%d" % c[:3] for c in SEEDED])
def test_contract_equals_the_reference_loops(h, w, n, seed):
    masks, scores = proposals(h, w, n, seed)
    assert len(set(scores.tolist())) == n and len({int((m != 0).sum()) for m in masks}) == n
    for src in (masks, masks != 0):                              # 0 / 255 bytes (255 * 255 wraps to 1) and bools
        ref_masks, ref_source = reference_nms_combine(src, scores)
        out, count, source, kept, ids, out_scores = mask_nms_np(src, scores)
        assert count == len(ref_masks) <= kept <= n
        assert source[:count].tolist() == ref_source and (source[count:] == -1).all()
        for k in range(count):
            np.testing.assert_array_equal(out[k] == 255, ref_masks[k])
        assert not out[count:].any() and set(np.unique(out)) <= {0, 255}
        np.testing.assert_array_equal(out_scores[:count], scores[source[:count]])
        assert (out_scores[count:] == 0).all()
        # disjoint, and the id map says the same
        assert ((out != 0).sum(0) <= 1).all()
        for k in range(count):
            np.testing.assert_array_equal(ids == k + 1, out[k] != 0)
        assert ids.dtype == np.int32 and ids.max(initial=0) == count


def test_seeded_sets_hold_duplicates_and_nested_masks():
    """The sets above are what they claim: some proposals are suppressed, some survivors hidden or partly covered."""
    suppressed = hidden = covered = 0
    for h, w, n, seed in SEEDED:
        masks, scores = proposals(h, w, n, seed)
        out, count, source, kept, _, _ = mask_nms_np(masks, scores)
        suppressed += n - kept
        hidden += kept - count
        covered += sum(int((out[k] != 0).sum()) < int((masks[source[k]] != 0).sum()) for k in range(count))
    assert suppressed >= 20 and covered >= 20 and hidden >= 1


# ---- hand-built cases (shared with the GPU tests) ----
def rows(h, w, *spans):
    """One mask per span (y0, y1, x0, x1) -> u8 [n,h,w] of 0 / 255."""
    m = np.zeros((len(spans), h, w), np.uint8)
    for k, (y0, y1, x0, x1) in enumerate(spans):
        m[k, y0:y1, x0:x1] = 255
    return m


def hand_cases():
    """name -> (masks, scores, {on_top: (count, kept, source[:count])})."""
    c = {}
    # IoU exactly 7 / 10: a 1 x 10 strip and its first 7 pixels.  float32(7) / float32(10) rounds to float32(0.7): kept - and then hidden
    # under the strip when the large one goes on top
    c["iou_7_10_kept"] = (rows(9, 20, (1, 2, 0, 10), (1, 2, 0, 7)), [0.9, 0.8], {"large": (1, 2, [0]), "small": (2, 2, [0, 1])})
    # IoU 71 / 101 > 0.7: suppressed
    m = np.zeros((2, 9, 20), np.uint8)
    m[0].ravel()[:101] = 255
    m[1].ravel()[:71] = 255
    c["iou_71_101_suppressed"] = (m, [0.9, 0.8], {"large": (1, 1, [0]), "small": (1, 1, [0])})
    # two empty masks: 0 / 0 = NaN suppresses the second; the survivor is never visible
    c["two_empty"] = (np.zeros((2, 9, 20), np.uint8), [0.5, 0.6], {"large": (0, 1, []), "small": (0, 1, [])})
    # one empty, one not: IoU 0, both survive the NMS, the empty one is absent from the output
    c["one_empty"] = (rows(9, 20, (0, 0, 0, 0), (2, 5, 3, 9)), [0.9, 0.1], {"large": (1, 2, [1]), "small": (1, 2, [1])})
    # equal scores: the higher index is visited first, so of two duplicates the SECOND survives
    c["equal_scores"] = (rows(9, 20, (2, 5, 3, 9), (2, 5, 3, 9), (6, 8, 0, 4)), [0.5, 0.5, 0.5],
                         {"large": (2, 2, [2, 1]), "small": (2, 2, [1, 2])})
    # equal areas, overlapping a little: painted in visit order (score), so the lower-scored one ends up on top under "large"
    c["equal_areas"] = (rows(9, 20, (1, 5, 2, 8), (3, 7, 4, 10)), [0.9, 0.3], {"large": (2, 2, [0, 1]), "small": (2, 2, [1, 0])})
    # a survivor completely hidden: a small mask inside a large one (IoU 6 / 60).  "small" keeps what "large" hides
    c["hidden_survivor"] = (rows(9, 20, (1, 7, 2, 12), (3, 5, 4, 7)), [0.4, 0.9], {"large": (1, 2, [0]), "small": (2, 2, [0, 1])})
    # a NaN score: that mask is not there
    c["absent_mask"] = (rows(9, 20, (1, 7, 2, 12), (1, 7, 2, 12), (0, 1, 0, 5)), [0.4, np.nan, 0.2], {"large": (2, 2, [2, 0]), "small": (2, 2, [0, 2])})
    return {k: (m, np.array(s, np.float32), w) for k, (m, s, w) in c.items()}


def test_seven_tenths_rounds_to_the_threshold():
    with np.errstate(all="raise"):
        assert np.float32(7) / ((np.float32(10) + np.float32(7)) - np.float32(7)) == np.float32(0.7)
        assert np.float32(71) / ((np.float32(101) + np.float32(71)) - np.float32(71)) > np.float32(0.7)


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_built_cases(name):
    masks, scores, want = hand_cases()[name]
    for on_top, (count, kept, source) in want.items():
        out, c, src, k, ids, out_scores = mask_nms_np(masks, scores, 0.7, on_top)
        assert (c, k, src[:c].tolist()) == (count, kept, source), (name, on_top, c, k, src)
        assert (src[c:] == -1).all() and not out[c:].any()
        assert ((out != 0).sum(0) <= 1).all()
        np.testing.assert_array_equal(out_scores[:c], scores[src[:c]])
    if name == "hidden_survivor":
        small = mask_nms_np(masks, scores, 0.7, "small")[0]
        np.testing.assert_array_equal(small[1], masks[1])                     # the nested mask, whole
        np.testing.assert_array_equal(small[0], masks[0] & ~masks[1])
        np.testing.assert_array_equal(mask_nms_np(masks, scores, 0.7, "large")[0][0], masks[0])
    if name == "equal_areas":
        large = mask_nms_np(masks, scores, 0.7, "large")[0]
        np.testing.assert_array_equal(large[1], masks[1])                     # painted last: whole
        np.testing.assert_array_equal(large[0], masks[0] & ~masks[1])


def test_no_masks_and_absent_masks():
    out, count, source, kept, ids, out_scores = mask_nms_np(np.zeros((0, 9, 20), np.uint8), np.zeros((0,), np.float32))
    assert out.shape == (0, 9, 20) and count == 0 and kept == 0 and source.shape == (0,) and not ids.any() and ids.shape == (9, 20)
    # NaN-scored masks are as good as dropped: the same output as the call without them, the sources in the caller's numbering
    masks, scores = proposals(24, 40, 12, 3, distinct=False)
    gone = np.array([1, 4, 5, 11])
    there = np.setdiff1d(np.arange(12), gone)
    s = scores.copy()
    s[gone] = np.nan
    a = mask_nms_np(masks, s)
    b = mask_nms_np(masks[there], scores[there])
    assert a[1] == b[1] and a[3] == b[3]
    np.testing.assert_array_equal(a[0][:a[1]], b[0][:b[1]])
    np.testing.assert_array_equal(a[2][:a[1]], there[b[2][:b[1]]])
    np.testing.assert_array_equal(a[4], b[4])


def test_ties_follow_the_stated_rule():
    """Equal scores and equal areas throughout: the contract is still a function of its inputs, and follows the rule it states."""
    masks, scores = proposals(24, 40, 16, 9, distinct=False)
    out, count, source, kept, ids, _ = mask_nms_np(masks, scores)
    assert len(set(scores.tolist())) <= 3
    order = np.argsort(scores, kind="stable")[::-1]
    for a, b in zip(order[:-1], order[1:]):
        assert scores[a] > scores[b] or (scores[a] == scores[b] and a > b)
    assert int(order[0]) in source[:count].tolist() or kept > count      # the first visited mask is always kept


# ---- the options and the argument checks that need no GPU ----
def test_masknms_options():
    a, b = MaskNMS(), MaskNMS(0.7, "large")
    assert a == b and hash(a) == hash(b) and a != MaskNMS(0.5) and a != MaskNMS(on_top="small")
    assert repr(MaskNMS(0.5, "small")) == "MaskNMS(thresh=0.5, on_top='small')"
    assert a.args() == (0.7, 0) and MaskNMS(on_top="small").args() == (0.7, 1)
    assert len({a, b, MaskNMS(0.5)}) == 2
    assert MaskNMS.parse(None) is None and MaskNMS.parse(a) is a
    for bad in (dict(thresh=-0.1), dict(thresh=1.5), dict(thresh=float("nan")), dict(thresh="0.7"), dict(thresh=True), dict(on_top="top"),
                dict(on_top=0)):
        with pytest.raises(ValueError):
            MaskNMS(**bad)
    for bad in (0.7, "large", True):
        with pytest.raises(ValueError):
            MaskNMS.parse(bad)
    assert MAX_MASKS == 1024


def test_scores_are_checked_on_the_host():
    s = check_scores([0.5, 1, 0.25], 3)
    assert s.dtype == np.float32 and s.flags.c_contiguous and s.tolist() == [0.5, 1.0, 0.25]
    assert check_scores(None, 0).shape == (0,)
    for bad, n in ((None, 2), ([0.5], 2), ([0.5, np.nan], 2), ([0.5, np.inf], 2), ([0.5, 1e39], 2), ([[0.5, 0.1]], 2), ([True, False], 2),
                   (["a", "b"], 2)):
        with pytest.raises(ValueError):
            check_scores(bad, n)


def test_predictor_refuses_missing_or_non_finite_scores_before_any_launch():
    """No GPU here: a call that got as far as building an engine would fail with another error than ValueError."""
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
    pred = MaskRefinerPredictor(None, device="cuda:0", nms=MaskNMS())
    assert pred.nms == MaskNMS() and pred.model.nms == MaskNMS()
    rgb = np.zeros((32, 48, 3), np.uint8)
    masks = rows(32, 48, (1, 9, 2, 12), (3, 9, 4, 17))
    with pytest.raises(ValueError, match="required"):
        pred.predict(rgb, rgb, masks)
    with pytest.raises(ValueError, match="finite"):
        pred.predict(rgb, rgb, masks, [0.5, float("nan")])
    with pytest.raises(ValueError, match="finite"):
        pred.predict(rgb, rgb, masks, mask_scores=[0.5, float("inf")])
    with pytest.raises(ValueError):
        pred.predict(rgb, rgb, masks, [0.5])
    with pytest.raises(ValueError, match="required"):
        pred.predict_batch(rgb[None], rgb[None], [masks])
    with pytest.raises(ValueError):
        pred.predict_batch(rgb[None], rgb[None], [masks], scores_list=[[0.5, 0.1], [0.3]])
    with pytest.raises(ValueError, match="required"):
        pred.model.enqueue_batch(None, None, None)
    with pytest.raises(ValueError):
        MaskRefinerPredictor(None, device="cuda:0", nms=0.7)


def test_abi_entry_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "quber_hip.h")).read()
    decl = re.search(r"int quber_mask_nms\(([^;]*)\);", txt)
    assert decl is not None
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    res, args = _lib.SIGNATURES["quber_mask_nms"]
    assert res is ctypes.c_int and len(args) == len(params) == 13
    assert [p.split()[-1] for p in params] == ["ctx", "dev_masks", "dev_scores", "batch", "n_masks", "thresh", "on_top", "dev_out_masks",
                                               "dev_ids", "dev_source", "dev_out_scores", "dev_report", "stream"]
    for p, a in zip(params, args):
        assert a is (ctypes.c_float if p.startswith("float ") else ctypes.c_int32 if p.startswith("int32_t ") else ctypes.c_void_p), p
    assert hasattr(_lib.load(), "quber_mask_nms")
    src = open(os.path.join(ROOT, "quber_amd", "csrc", "masknms.hip")).read()
    assert int(re.search(r"constexpr int MN_MAX = (\d+);", src).group(1)) == MAX_MASKS
