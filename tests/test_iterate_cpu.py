"""CPU: iterative refinement (INTEGRATION.md "Iterative refinement") - the contract of the three kernels of csrc/iterate.hip and of the
loop's bookkeeping in numpy (tests/test_gpu_iterate.py compares the HIP path against these), their self-checks on hand-made cases,
the ABI entries and public constructors, and the soundness of the GPU tests' inputs on the oracle alone."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from quber_amd import _lib, arch

TOP_K = 200


# ---- the contract ----
def relabel_np(panoptic, labels, count, mirror=False):
    """panoptic f32 [B,H,W], labels f32 [B,top_k], count [B] -> ids i32 [B,H,W] ([2B,H,W] with the W-mirrors behind the batch):
    1 + the first position of the pixel's value in labels[b][:count[b]], 0 when it is not there."""
    pan = np.asarray(panoptic, np.float32)
    labels = np.asarray(labels, np.float32)
    ids = np.zeros(pan.shape, np.int32)
    for b in range(pan.shape[0]):
        n = min(max(int(count[b]), 0), labels.shape[1])
        for j in range(n - 1, -1, -1):                   # descending: the first position wins
            ids[b][pan[b] == labels[b, j]] = j + 1
    return np.concatenate([ids, ids[:, :, ::-1]]) if mirror else ids


def overlap_masks_np(masks, ids, n_ids):
    """masks [B,N,H,W] (non-zero = inside), ids i32 [B,H,W] -> (table i64 [B,N,n_ids+1], area i64 [B,n_ids+1]); a pixel whose id
    lies outside 0..n_ids is counted nowhere."""
    masks, ids = np.asarray(masks), np.asarray(ids)
    B, N = masks.shape[:2]
    table = np.zeros((B, N, n_ids + 1), np.int64)
    area = np.zeros((B, n_ids + 1), np.int64)
    for b in range(B):
        ok = (ids[b] >= 0) & (ids[b] <= n_ids)
        area[b] = np.bincount(ids[b][ok], minlength=n_ids + 1)
        for n in range(N):
            table[b, n] = np.bincount(ids[b][ok & (masks[b, n] != 0)], minlength=n_ids + 1)
    return table, area


def overlap_ids_np(a, b, n_a, n_b):
    """a, b i32 [B,H,W] -> i64 [B,n_a+1,n_b+1]: pixels with a == i and b == j; out-of-range ids counted nowhere."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    out = np.zeros((a.shape[0], n_a + 1, n_b + 1), np.int64)
    for f in range(a.shape[0]):
        ok = (a[f] >= 0) & (a[f] <= n_a) & (b[f] >= 0) & (b[f] <= n_b)
        out[f] = np.bincount(a[f][ok] * (n_b + 1) + b[f][ok], minlength=(n_a + 1) * (n_b + 1)).reshape(n_a + 1, n_b + 1)
    return out


def same_segmentation_np(table):
    """table [n_a+1,n_b+1] (row / column 0 = no instance): the two label maps describe the same segmentation iff every row and every
    column holds at most one non-zero cell and row 0 / column 0 none besides [0][0]."""
    nz = np.asarray(table) != 0
    return bool((nz.sum(1) <= 1).all() and (nz.sum(0) <= 1).all() and not nz[0, 1:].any() and not nz[1:, 0].any())


def match_initial_np(table, area):
    """table [N,K+1] / area [K+1] of one frame -> (initial_overlap i64 [N,K+1], initial_index i64 [K], initial_iou f32 [K]): per
    instance the initial mask of the largest IoU = inter / (|mask| + area - inter) in float64, the first index wins ties; -1 / 0
    when no initial mask touches the instance.  |mask| is the row sum: every pixel of a mask has some id."""
    table, area = np.asarray(table).astype(np.int64), np.asarray(area).astype(np.int64)
    N, K = table.shape[0], table.shape[1] - 1
    index = np.full((K,), -1, np.int64)
    iou = np.zeros((K,), np.float32)
    size = table.sum(1)
    for k in range(K):
        best = 0.0
        for n in range(N):
            inter = int(table[n, k + 1])
            if inter == 0:
                continue
            v = np.float64(inter) / np.float64(int(size[n]) + int(area[k + 1]) - inter)
            if v > best:
                best, index[k] = v, n
        iou[k] = np.float32(best)
    return table, index, iou


# ---- self-checks on hand-made cases ----
def _two_blobs():
    a = np.zeros((1, 6, 8), np.int32)
    a[0, 1:3, 1:4] = 1
    a[0, 3:6, 4:8] = 2
    return a


def test_relabel_np_cases():
    pan = np.full((2, 3, 4), -1, np.float32)
    pan[0, 0, :2] = 1000
    pan[0, 1, 1:] = 1003
    pan[0, 2, 0] = 1001                                  # not in the list
    pan[1, :, 3] = 1002                                  # behind count[1]
    labels = np.full((2, 5), 1002, np.float32)
    labels[0, :2] = (1000, 1003)
    ids = relabel_np(pan, labels, [2, 0])
    assert ids.dtype == np.int32 and ids[0].tolist() == [[1, 1, 0, 0], [0, 2, 2, 2], [0, 0, 0, 0]] and not ids[1].any()
    m = relabel_np(pan, labels, [2, 0], mirror=True)
    assert m.shape == (4, 3, 4) and np.array_equal(m[:2], ids) and np.array_equal(m[2:], ids[:, :, ::-1])
    assert relabel_np(pan, labels, [0, 9])[1, :, 3].tolist() == [1, 1, 1]          # count above top_k counts as top_k; first position


def test_same_segmentation_np_cases():
    a = _two_blobs()
    T = lambda x, y: overlap_ids_np(x, y, 3, 3)[0]
    assert same_segmentation_np(T(a, a))
    perm = np.where(a == 1, 3, np.where(a == 2, 1, 0)).astype(np.int32)            # permuted labels
    assert same_segmentation_np(T(a, perm)) and same_segmentation_np(T(perm, a))
    moved = a.copy()
    moved[0, 1, 1] = 0                                   # one pixel moved to the background
    assert not same_segmentation_np(T(a, moved)) and not same_segmentation_np(T(moved, a))
    split = a.copy()
    split[0, 3:6, 6:8] = 3
    assert not same_segmentation_np(T(a, split))
    assert not same_segmentation_np(T(split, a))         # the merge
    gone = np.where(a == 2, 0, a).astype(np.int32)       # an instance vanished into the background
    assert not same_segmentation_np(T(a, gone)) and not same_segmentation_np(T(gone, a))
    full = np.ones((1, 6, 8), np.int32)                  # no background: row / column 0 empty
    t = T(full, full * 2)
    assert t[0].sum() == 0 and t[:, 0].sum() == 0 and same_segmentation_np(t)
    assert not same_segmentation_np(T(full, a))
    assert T(a, a).sum() == 48
    bad = a.copy()
    bad[0, 0, 0] = 7                                     # out of range: counted nowhere
    assert T(bad, a).sum() == 47


def test_overlap_masks_and_match_initial_np_cases():
    ids = _two_blobs()                                   # areas: background 30, id 1: 6, id 2: 12
    masks = np.zeros((1, 4, 6, 8), np.uint8)
    masks[0, 0, 3:6, 4:8] = 255                          # exactly instance 2
    masks[0, 1, 1:3, 0:3] = 7                            # 4 of instance 1, 2 dropped
    masks[0, 2, 0:6, 0:8] = 1                            # everything; overlaps the others
    table, area = overlap_masks_np(masks, ids, 2)
    assert area.tolist() == [[30, 6, 12]]
    assert table[0].tolist() == [[0, 0, 12], [2, 4, 0], [30, 6, 12], [0, 0, 0]]
    assert (table.sum(2) == (masks != 0).sum((2, 3))).all()
    ov, index, iou = match_initial_np(table[0], area[0])
    assert ov is not None and index.tolist() == [1, 0] and iou.dtype == np.float32
    assert iou[0] == np.float32(4 / 8) and iou[1] == np.float32(1.0)
    # a tie goes to the first index; an instance nobody touches: -1 / 0; no masks at all
    tie = np.array([[0, 3], [0, 3]])
    assert match_initial_np(tie, np.array([0, 3]))[1].tolist() == [0]
    ov, index, iou = match_initial_np(np.array([[5, 0, 1]]), np.array([9, 4, 1]))
    assert index.tolist() == [-1, 0] and iou[0] == 0 and iou[1] == np.float32(1 / 6)
    ov, index, iou = match_initial_np(np.zeros((0, 3), np.int64), np.array([1, 2, 3]))
    assert ov.shape == (0, 3) and index.tolist() == [-1, -1] and iou.tolist() == [0, 0]


def test_torch_bookkeeping_equals_the_contract():
    """same_segmentation / match_initial of the predictor (torch, run on the device there) against the numpy statement."""
    from quber_amd.maskrefiner.predictor import match_initial, same_segmentation
    rng = np.random.default_rng(3)
    tabs = []
    for i in range(40):
        n = int(rng.integers(1, 6))
        t = np.zeros((6, 6), np.int64)
        p = rng.permutation(5)[:n]
        for j in range(n):
            t[j + 1, p[j] + 1] = rng.integers(1, 50)
        t[0, 0] = rng.integers(0, 2) * 10
        if i % 3 == 1:
            t[rng.integers(0, 6), rng.integers(0, 6)] += 1
        if i % 3 == 2:
            t[0, rng.integers(1, 6)] += rng.integers(0, 2)
        tabs.append(t)
    got = same_segmentation(torch.from_numpy(np.stack(tabs)))
    want = [same_segmentation_np(t) for t in tabs]
    assert got.tolist() == want and any(want) and not all(want)
    for i in range(30):
        N, K = int(rng.integers(0, 7)), int(rng.integers(0, 6))
        cap_n, cap_k = N + 2, K + 3
        table = np.zeros((cap_n, cap_k + 1), np.int32)
        table[:N, :K + 1] = rng.integers(0, 4, (N, K + 1)) * rng.integers(0, 2, (N, K + 1))
        area = np.zeros((cap_k + 1,), np.int32)
        area[:K + 1] = table[:N, :K + 1].max(0, initial=0) + rng.integers(1, 3, K + 1)
        ov, idx, iou = match_initial(torch.from_numpy(table), torch.from_numpy(area), N, K)
        ov_np, idx_np, iou_np = match_initial_np(table[:N, :K + 1], area[:K + 1])
        assert ov.dtype == torch.int64 and idx.dtype == torch.int64 and iou.dtype == torch.float32
        np.testing.assert_array_equal(ov.numpy(), ov_np)
        np.testing.assert_array_equal(idx.numpy(), idx_np)
        np.testing.assert_array_equal(iou.numpy().view(np.uint32), iou_np.view(np.uint32))


# ---- ABI and public interface ----
NEW = ("quber_relabel_panoptic", "quber_overlap_masks", "quber_overlap_ids")


def test_header_signatures_and_library_hold_the_three_entries():
    txt = open(os.path.join(ROOT, "include", "quber_hip.h")).read()
    P, I = _lib._P, _lib._I
    assert re.search(r"int quber_relabel_panoptic\(quber_ctx\* ctx, const float\* dev_panoptic, const float\* dev_labels, "
                     r"const int32_t\* dev_count,\s+int32_t batch, int32_t mirror, int32_t\* dev_ids, void\* stream\);", txt)
    assert re.search(r"int quber_overlap_masks\(quber_ctx\* ctx, const uint8_t\* dev_masks, const int32_t\* dev_ids, int32_t batch, "
                     r"int32_t n_masks,\s+int32_t n_ids, uint32_t\* dev_table, uint32_t\* dev_area, void\* stream\);", txt)
    assert re.search(r"int quber_overlap_ids\(quber_ctx\* ctx, const int32_t\* dev_a, const int32_t\* dev_b, int32_t batch, int32_t n_a, "
                     r"int32_t n_b,\s+uint32_t\* dev_table, void\* stream\);", txt)
    assert _lib.SIGNATURES["quber_relabel_panoptic"] == (ctypes.c_int, [P, P, P, P, I, I, P, P])
    assert _lib.SIGNATURES["quber_overlap_masks"] == (ctypes.c_int, [P, P, P, I, I, I, P, P, P])
    assert _lib.SIGNATURES["quber_overlap_ids"] == (ctypes.c_int, [P, P, P, I, I, I, P, P])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    loaded = _lib.load()
    assert loaded.quber_relabel_panoptic(None, None, None, None, 1, 0, None, None) != 0
    assert b"null context" in loaded.quber_last_error()
    assert loaded.quber_overlap_masks(None, None, None, 1, 0, 0, None, None, None) != 0
    assert loaded.quber_overlap_ids(None, None, None, 1, 0, 0, None, None) != 0


def test_constructors_take_the_iteration_keywords():
    from quber_amd.eval.refiner_model import MaskRefiner, MaskRefinerTTA
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor, RefinerModel
    for cls in (MaskRefinerPredictor, MaskRefiner, RefinerModel):
        p = inspect.signature(cls.__init__).parameters
        assert p["iterations"].default == 1 and p["until_converged"].default is False and p["track_initial"].default is False, cls
    inspect.signature(MaskRefinerTTA.__init__).bind(None, "configs/x.yaml", iterations=3, until_converged=True, track_initial=True)
    # the trailing keywords leave the existing positional / keyword uses alone
    m = RefinerModel(None, {}, "cpu", tta=True)
    assert (m.iterations, m.until_converged, m.track_initial, m.tta) == (1, False, False, True)
    m = RefinerModel(None, {}, "cpu", iterations=3, until_converged=True, track_initial=True)
    assert (m.iterations, m.until_converged, m.track_initial, m.top_k) == (3, True, True, TOP_K)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            RefinerModel(None, {}, "cpu", iterations=bad)
        with pytest.raises(ValueError):
            MaskRefinerPredictor(None, device="cpu", state_dict={}, iterations=bad)
        with pytest.raises(ValueError):
            MaskRefiner(None, iterations=bad)


# ---- the inputs of the GPU tests, on the oracle alone ----
def fixed_point_state_dict():
    """Weights whose refinement is a fixed point by construction: the foreground / centre / offset predictors ignore their features
    (weights 0, biases +4 / -4 / 0), so every pixel is foreground, no centre passes the threshold and the frame is one instance -
    the K = 0 "stuff blob", label 1000 - whatever the initial masks were."""
    sd = arch.init_state_dict(seed=1, loud_heads=True)
    for name, bias in (("foreground", 4.0), ("center", -4.0), ("offset", 0.0)):
        w = [k for k in sd if k.endswith(f"{name}_predictor.predictor.weight")]
        b = [k for k in sd if k.endswith(f"{name}_predictor.predictor.bias")]
        assert len(w) == 1 and len(b) == 1, name
        sd[w[0]] = np.zeros_like(sd[w[0]])
        sd[b[0]] = np.full_like(sd[b[0]], bias)
    return sd


def oracle_pass(net, image, masks):
    """One pass on the oracle: masks u8 [N,H,W] -> (heads of the oracle network, oracle/postproc_ref.postprocess of them)."""
    from oracle import encode_np, postproc_ref
    offs = encode_np.encode_initial_masks(np.asarray(masks, np.uint8))
    with torch.no_grad():
        ref = net(image, torch.from_numpy(offs[None]))
    return ref, postproc_ref.postprocess(ref["foreground"][0], ref["center"][0], ref["offset"][0])


def ids_of(o, top_k=TOP_K):
    """The compact ids of a postproc_ref result, through the contract."""
    k = len(o["labels"])
    labels = np.zeros((1, top_k), np.float32)
    labels[0, :k] = o["labels"].numpy()
    return relabel_np(o["panoptic"].numpy()[None], labels, [k])[0]


def test_fixed_point_inputs_on_the_oracle():
    from test_gpu_loud_parity import _oracle, _scene
    h, w = 96, 128
    batch, offs, image = _scene(5, 1, h, w, 3)
    net = _oracle(fixed_point_state_dict())
    masks = batch["masks"][0]
    maps = []
    for p in range(3):
        ref, o = oracle_pass(net, image, masks)
        assert o["labels"].tolist() == [1000.0] and int(o["masks"].sum()) == h * w, p
        maps.append(ids_of(o))
        masks = o["masks"].numpy().astype(np.uint8) * 255
    assert all(np.array_equal(maps[0], m) for m in maps[1:]) and (maps[0] == 1).all()
    assert same_segmentation_np(overlap_ids_np(maps[0][None], maps[1][None], TOP_K, TOP_K)[0])
    # what track_initial reports for this frame: every initial mask lies inside the one instance
    table, area = overlap_masks_np(batch["masks"], maps[-1][None], TOP_K)
    ov, index, iou = match_initial_np(table[0][:, :2], area[0][:2])
    sizes = (batch["masks"][0] != 0).sum((1, 2))
    assert ov[:, 1].tolist() == sizes.tolist() and index.tolist() == [int(np.argmax(sizes))]
    assert iou[0] == np.float32(np.float64(sizes.max()) / np.float64(h * w))
