"""CPU: the connected-component clean-up of the refined instances (INTEGRATION.md "Connected-component clean-up"; csrc/cleanup.hip).

The contract in numpy (``cleanup_np`` / ``cleanup_post_np``: tests/test_gpu_cleanup.py compares the HIP path against them, exactly), its
self-checks on hand-drawn maps, the equivalence of the two presets with the functions the reference's competing refiners call, the ABI
entries and the public constructors, and the scenes the GPU tests run.

``largest_connected_component_np`` and ``remove_small_regions_np`` restate eval/utilities.py:726-748 and eval/refiner_model.py:526-549
with ``scipy.ndimage.label`` in place of ``cv2.connectedComponents[WithStats]`` (OpenCV is not installed).  Both labellers number the
components in the order a raster scan meets their first pixel, so "the first maximum" (the reference's strict ``>`` and its
``np.argmax``) is the component whose first pixel comes first; for scipy that order is checked below
(test_contract_hand_drawn_cases: the tie), for cv2 the agreement on ties is ARGUED - from its scan-order label assignment - and not
tested here."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from conftest import ROOT
from quber_amd import _lib
from quber_amd.cleanup import Cleanup


def _structure(connectivity):
    return ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)


# ---- the contract ----
def cleanup_np(ids, n_ids, connectivity=8, keep_largest=False, min_island_area=0, max_hole_area=0):
    """ids int [B,H,W] -> (cleaned ids i32 [B,H,W], report i64 [B,n_ids+1,4]).
    A value outside 0..n_ids counts as 0.  Frames never interact.
    Step 1: per id i >= 1 the c-connected components of {ids == i}, in raster order of their first pixel; the largest = most pixels,
    the earlier among equals.  keep_largest: all others become 0; else those with fewer than min_island_area pixels do, the largest
    never.  Step 2 (max_hole_area > 0, on the result of step 1): a c-connected component of {ids == 0} becomes i iff it has fewer
    than max_hole_area pixels and its c-neighbours outside itself all carry i.
    report[b, i] = (components of i, pixels removed, pixels gained, final area); report[b, 0] = (void components examined in step
    2, 0, pixels filled in all, final void area)."""
    ids = np.asarray(ids)
    out = np.where((ids >= 0) & (ids <= n_ids), ids, 0).astype(np.int32)
    st = _structure(connectivity)
    report = np.zeros((out.shape[0], n_ids + 1, 4), np.int64)
    for b in range(out.shape[0]):
        m = out[b]
        src = m.copy()
        for i in np.unique(src[src > 0]):
            lab, n = ndimage.label(src == i, structure=st)
            sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
            largest = int(np.argmax(sizes)) + 1              # the first maximum: the lowest label = the earliest first pixel
            drop = [j for j in range(1, n + 1) if j != largest and (keep_largest or sizes[j - 1] < min_island_area)]
            report[b, i, 0] = n
            if drop:
                sel = np.isin(lab, drop)
                report[b, i, 1] = int(sel.sum())
                m[sel] = 0
        if max_hole_area > 0:
            src = m.copy()
            lab, n = ndimage.label(src == 0, structure=st)
            report[b, 0, 0] = n
            for j, sl in enumerate(ndimage.find_objects(lab), 1):
                win = tuple(slice(max(s.start - 1, 0), s.stop + 1) for s in sl)
                comp = lab[win] == j
                size = int(comp.sum())
                if size >= max_hole_area:
                    continue
                around = np.unique(src[win][ndimage.binary_dilation(comp, structure=st) & ~comp])   # never 0: the component is maximal
                if len(around) == 1:
                    m[win][comp] = around[0]
                    report[b, around[0], 2] += size
                    report[b, 0, 2] += size
        report[b, :, 3] = np.bincount(m.ravel(), minlength=n_ids + 1)
    return out, report


def cleanup_post_np(logits, panoptic, labels, count, opts):
    """The contract of quber_cleanup_postprocess on host copies of the tables of quber_postprocess: logits f32 [B,planes,H,W],
    panoptic f32 [B,H,W], labels f32 [B,cap], count [B] -> (panoptic, scores f32 [B,cap], boxes f32 [B,cap,4], report): compact ids
    (relabel_np), clean-up with n_ids = cap, labels written back (-1 where the id is 0), then per instance
    score = f32(mean of f64(f32 sigmoid(fg)) over the mask) * centre plane at the truncated f32 centre of mass, box = min / max + 1."""
    from test_iterate_cpu import relabel_np
    logits = np.asarray(logits, np.float32)
    labels = np.asarray(labels, np.float32)
    B, cap = labels.shape
    c, keep, a_i, a_h = opts.args()
    ids, report = cleanup_np(relabel_np(panoptic, labels, count), cap, c, bool(keep), a_i, a_h)
    pan = np.full(ids.shape, -1, np.float32)
    scores = np.zeros((B, cap), np.float32)
    boxes = np.zeros((B, cap, 4), np.float32)
    for b in range(B):
        prob = (np.float32(1) / (np.float32(1) + np.exp(-logits[b, 0]))).astype(np.float32)
        for j in range(min(max(int(count[b]), 0), cap)):
            sel = ids[b] == j + 1
            pan[b][sel] = labels[b, j]
            ys, xs = np.nonzero(sel)
            if len(ys) == 0:
                continue
            sem = np.float32(prob[sel].astype(np.float64).sum() / np.float64(len(ys)))
            my, mx = np.float32(np.float64(ys.sum()) / len(ys)), np.float32(np.float64(xs.sum()) / len(ys))
            scores[b, j] = sem * logits[b, 1, int(my), int(mx)]
            boxes[b, j] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
    return pan, scores, boxes, report


# ---- the two functions of the reference, restated ----
def largest_connected_component_np(mask, connectivity=4):
    """eval/utilities.py:726-748: the component with strictly more pixels than every component labelled before it."""
    lab, n = ndimage.label(np.asarray(mask) != 0, structure=_structure(connectivity))
    pick, most = -1, -1
    for j in range(1, n + 1):
        size = np.count_nonzero(lab == j)
        if size > most:
            pick, most = j, size
    return (lab == pick).astype(np.asarray(mask).dtype)


def remove_small_regions_np(mask, area_thresh, mode):
    """eval/refiner_model.py:526-549, 8-connected.  "islands": the components of the mask smaller than area_thresh go, but if all are
    that small the first largest stays; "holes": the components of the complement smaller than area_thresh join the mask.
    -> (mask, changed)."""
    assert mode in ("holes", "islands")
    mask = np.asarray(mask).astype(bool)
    lab, n = ndimage.label(~mask if mode == "holes" else mask, structure=_structure(8))
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    small = np.flatnonzero(sizes < area_thresh) + 1
    if len(small) == 0:
        return mask, False
    if mode == "holes":
        return mask | np.isin(lab, small), True
    keep = np.setdiff1d(np.arange(1, n + 1), small)
    if len(keep) == 0:
        keep = [int(np.argmax(sizes)) + 1]
    return np.isin(lab, keep), True


# ---- maps ----
def blocky(rng, shape, values, cell=7, noise=0.02):
    """[B,H,W] drawn from `values`: constant cells with a sprinkle of single pixels."""
    B, H, W = shape
    coarse = rng.integers(0, len(values), (B, -(-H // cell), -(-W // cell)))
    idx = np.kron(coarse, np.ones((1, cell, cell), np.int64))[:, :H, :W]
    flip = rng.random(shape) < noise
    idx[flip] = rng.integers(0, len(values), int(flip.sum()))
    return np.asarray(values)[idx].astype(np.int32)


def _draw(rows):
    return np.array([[int(c, 36) if c != "." else 0 for c in r] for r in rows], np.int32)[None]


# hand-drawn cases: name -> (map, n_ids, (connectivity, keep_largest, min_island_area, max_hole_area), expected map, expected report rows)
TIE = _draw(["11.11.111",
             ".........",
             "111.2...."])                                   # three components of 1; two of three pixels: the raster-first one wins
HAND = {
    "tie-raster-first": (TIE, 2, (4, True, 0, 0), _draw(["......111", ".........", "....2...."]),
                         {1: (4, 7, 0, 3), 2: (1, 0, 0, 1), 0: (0, 0, 0, 23)}),
    "island-of-exactly-a-stays": (TIE, 2, (4, False, 3, 0), _draw(["......111", ".........", "111.2...."]),
                                  {1: (4, 4, 0, 6), 2: (1, 0, 0, 1)}),
    "all-small-largest-stays": (TIE, 2, (4, False, 9, 0), _draw(["......111", ".........", "....2...."]), {1: (4, 7, 0, 3), 2: (1, 0, 0, 1)}),
    "zero-area-removes-nothing": (TIE, 2, (8, False, 0, 0), TIE, {1: (4, 0, 0, 10), 2: (1, 0, 0, 1)}),
    # holes: inside (2 px), at the frame edge (1 px), of exactly a_h = 3 px (stays), the long one between the instances (too large)
    "holes": (_draw(["11111.222",
                     "1..11.222",
                     "11111.2.2",
                     ".1111.222",
                     "11..1.222",
                     "11.11.222"]), 2, (4, False, 0, 3),
              _draw(["11111.222",
                     "11111.222",
                     "11111.222",
                     "11111.222",
                     "11..1.222",
                     "11.11.222"]), {0: (5, 0, 4, 9), 1: (1, 0, 3, 27), 2: (1, 0, 1, 18)}),
    # one and two void pixels that touch both instances, far below a_h: not filled; the single pixel inside 2 is
    "hole-between-two-instances": (_draw(["111222",
                                          "11.222",
                                          "111222",
                                          "11..22",
                                          "111222",
                                          "1112.2"]), 2, (4, False, 0, 100),
                                   _draw(["111222",
                                          "11.222",
                                          "111222",
                                          "11..22",
                                          "111222",
                                          "111222"]), {0: (3, 0, 1, 3), 1: (1, 0, 0, 16), 2: (1, 0, 1, 17)}),
    "all-void-is-not-a-hole": (_draw(["...", "..."]), 3, (8, False, 0, 100), _draw(["...", "..."]), {0: (1, 0, 0, 6)}),
    # a speck of 2 inside 1 is removed by step 1 and becomes 1 in step 2; the diagonal pixel of 1 is a component of its own for c = 4
    "speck-inside": (_draw(["11111....",
                            "12111.222",
                            "11111.222",
                            ".....1..."]), 2, (4, True, 0, 2),
                     _draw(["11111....",
                            "11111.222",
                            "11111.222",
                            "........."]), {0: (2, 0, 1, 15), 1: (2, 1, 1, 15), 2: (2, 1, 0, 6)}),
    "diagonal-joins-for-8": (_draw(["11111....",
                                    "12111.222",
                                    "11111.222",
                                    ".....1..."]), 2, (8, True, 0, 2),
                             _draw(["11111....",
                                    "11111.222",
                                    "11111.222",
                                    ".....1..."]), {0: (2, 0, 1, 14), 1: (1, 0, 1, 16), 2: (2, 1, 0, 6)}),
    "out-of-range-is-void": (np.array([[[1, 5, -1, 1], [255, 1, 70000, 1]]], np.int32), 1, (4, True, 0, 0),
                             _draw(["...1", "...1"]), {1: (3, 2, 0, 2), 0: (0, 0, 0, 6)}),
}


def test_contract_hand_drawn_cases():
    for name, (ids, n, o, want, rows) in HAND.items():
        got, rep = cleanup_np(ids, n, *o)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, got)
        for i, row in rows.items():
            assert tuple(rep[0, i]) == row, (name, i, rep[0])
        assert rep[0, :, 3].sum() == ids[0].size and (rep[0, 1:, 3] > 0).sum() == len(np.unique(got[got > 0])), name
        again, rep2 = cleanup_np(got, n, *o)
        assert np.array_equal(again, got) and not rep2[0, :, 1:3].any(), name


def test_frames_never_interact():
    a = np.zeros((2, 3, 5), np.int32)
    a[0, 2, 2:] = 1                                          # ends at the last pixel of frame 0 ...
    a[1, 0, :2] = 1                                          # ... frame 1 starts with two more
    a[1, 2, :] = 1
    got, rep = cleanup_np(a, 1, 4, True)
    assert got[0].sum() == 3 and got[1].sum() == 5 and rep[:, 1, 0].tolist() == [1, 2] and rep[:, 1, 1].tolist() == [0, 2]


# ---- the presets against the reference's functions ----
def _random_maps(seed, n_ids=6, shape=(3, 40, 61)):
    rng = np.random.default_rng(seed)
    return blocky(rng, shape, [0, 0] + list(range(1, n_ids + 1)), cell=int(rng.integers(3, 9)), noise=0.06)


@pytest.mark.parametrize("seed", range(6))
def test_uois_preset_is_largest_connected_component(seed):
    ids = _random_maps(seed)
    if seed == 0:                                            # ties between the largest components
        ids[:] = 0
        ids[:, 5:8, 5:9] = 1
        ids[:, 20:24, 30:33] = 1
        ids[:, 30:32, 2:8] = 1
        ids[0, 0, 0] = 2
        ids[0, 39, 60] = 2
    o = Cleanup.uois()
    assert o.args() == (4, 1, 0, 0)
    out, rep = cleanup_np(ids, 6, *o.args())
    ties = 0
    for b in range(ids.shape[0]):
        for i in range(1, 7):
            np.testing.assert_array_equal(out[b] == i, largest_connected_component_np(ids[b] == i, 4).astype(bool))
            lab, n = ndimage.label(ids[b] == i, structure=_structure(4))
            sizes = np.bincount(lab.ravel())[1:]
            ties += n > 1 and (sizes == sizes.max()).sum() > 1
    assert ties > 0 or seed != 0
    assert (rep[:, 1:, 0] > 1).any()


@pytest.mark.parametrize("seed,area", [(10, 4), (11, 12), (12, 30), (13, 10 ** 6)])
def test_islands_are_remove_small_regions_islands(seed, area):
    ids = _random_maps(seed)
    out, rep = cleanup_np(ids, 6, 8, False, area, 0)
    kept_all_small = 0
    for b in range(ids.shape[0]):
        for i in range(1, 7):
            want, _ = remove_small_regions_np(ids[b] == i, area, "islands")
            np.testing.assert_array_equal(out[b] == i, want)
            kept_all_small += area == 10 ** 6 and want.any()
    assert rep[:, 1:, 1].sum() > 0 and (area != 10 ** 6 or kept_all_small > 0)       # the keep-the-largest branch ran


def _nested_free_maps(seed, area, shape=(2, 48, 70)):
    """Instances as rectangles apart from each other (some touching side by side, some at the frame edge) with void holes of 1 .. 2 *
    area pixels punched into them: nothing but void lies inside a small complement component of an instance."""
    rng = np.random.default_rng(seed)
    B, H, W = shape
    ids = np.zeros(shape, np.int32)
    for b in range(B):
        i = 0
        for y0 in range(0, H - 14, 16):
            for x0 in range(0, W - 20, 23):
                i += 1
                ids[b, y0 + int(rng.integers(0, 3)):y0 + 14, x0 + int(rng.integers(0, 3)):x0 + 20 + 3 * (i % 2)] = i
                for _ in range(3):
                    hy, hx = y0 + int(rng.integers(3, 10)), x0 + int(rng.integers(3, 15))
                    hh, hw = int(rng.integers(1, 4)), int(rng.integers(1, max(2, 2 * area // 3)))
                    ids[b, hy:hy + hh, hx:hx + hw][ids[b, hy:hy + hh, hx:hx + hw] == i] = 0
    return ids, i


@pytest.mark.parametrize("seed,area", [(20, 3), (21, 6), (22, 10)])
def test_holes_against_remove_small_regions_holes(seed, area):
    o = Cleanup.sam(area)
    assert o.args() == (8, 0, 0, area) and Cleanup.sam().args() == (8, 0, 0, 300)
    # any map: what the clean-up gives an instance is part of what the reference's function gives it
    ids = _random_maps(seed)
    out, rep = cleanup_np(ids, 6, *o.args())
    for b in range(ids.shape[0]):
        for i in range(1, 7):
            want, _ = remove_small_regions_np(ids[b] == i, area, "holes")
            assert not ((out[b] == i) & ~want).any()
    assert rep[:, 0, 2].sum() > 0
    # maps on which no instance lies inside a small complement component of another: equality
    ids, n = _nested_free_maps(seed, area)
    out, rep = cleanup_np(ids, n, *o.args())
    filled = 0
    for b in range(ids.shape[0]):
        for i in range(1, n + 1):
            # (the construction property, on the oracle alone)
            lab, k = ndimage.label(ids[b] != i, structure=_structure(8))
            sizes = np.bincount(lab.ravel(), minlength=k + 1)
            for j in range(1, k + 1):
                assert sizes[j] >= area or not ids[b][lab == j].any(), (b, i, j)
            want, _ = remove_small_regions_np(ids[b] == i, area, "holes")
            np.testing.assert_array_equal(out[b] == i, want)
            filled += int((want & (ids[b] != i)).sum())
    assert filled > 0 and filled == rep[:, 0, 2].sum()
    assert (rep[:, 0, 0] > 1).all()                          # holes that stayed: too large


@pytest.mark.parametrize("o", [(4, True, 0, 0), (8, True, 0, 25), (8, False, 9, 0), (4, False, 5, 7), (8, False, 0, 300), (4, True, 0, 300)])
def test_idempotent(o):
    for seed in (30, 31):
        ids = _random_maps(seed)
        once, rep = cleanup_np(ids, 6, *o)
        twice, rep2 = cleanup_np(once, 6, *o)
        np.testing.assert_array_equal(twice, once)
        assert not rep2[:, :, 1:3].any() and np.array_equal(rep2[:, :, 3], rep[:, :, 3])
        assert (rep[:, 1:, 3] > 0).sum() == sum(len(np.unique(f[f > 0])) for f in ids)       # every instance keeps a pixel
        if o[1]:
            assert (rep2[:, 1:, 0] <= 1).all()


# ---- ABI and public interface ----
def test_header_signatures_and_library_hold_the_two_entries():
    txt = open(os.path.join(ROOT, "include", "quber_hip.h")).read()
    P, I = _lib._P, _lib._I
    assert re.search(r"int quber_cleanup_ids\(quber_ctx\* ctx, int32_t\* dev_ids, int32_t batch, int32_t n_ids, int32_t connectivity, "
                     r"int32_t keep_largest,\s+int32_t min_island_area, int32_t max_hole_area, uint32_t\* dev_report, void\* stream\);", txt)
    assert re.search(r"int quber_cleanup_postprocess\(quber_ctx\* ctx, const float\* dev_logits, int32_t n_planes, int32_t batch, "
                     r"float\* dev_panoptic,\s+const float\* dev_labels, const int32_t\* dev_count, float\* dev_scores, float\* dev_boxes,\s+"
                     r"int32_t connectivity, int32_t keep_largest, int32_t min_island_area, int32_t max_hole_area,\s+"
                     r"uint32_t\* dev_report, void\* stream\);", txt)
    assert _lib.SIGNATURES["quber_cleanup_ids"] == (ctypes.c_int, [P, P, I, I, I, I, I, I, P, P])
    assert _lib.SIGNATURES["quber_cleanup_postprocess"] == (ctypes.c_int, [P, P, I, I, P, P, P, P, P, I, I, I, I, P, P])
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("quber_cleanup_ids", "quber_cleanup_postprocess"):
        assert hasattr(lib, name), name
    loaded = _lib.load()
    assert loaded.quber_cleanup_ids(None, None, 1, 0, 8, 0, 0, 0, None, None) != 0
    assert b"null context" in loaded.quber_last_error()
    assert loaded.quber_cleanup_postprocess(None, None, 8, 1, None, None, None, None, None, 8, 0, 0, 0, None, None) != 0
    assert b"null context" in loaded.quber_last_error()
    mk = open(os.path.join(ROOT, "quber_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bcleanup\.hip\b", mk, re.M)


def test_options_class():
    o = Cleanup()
    assert (o.keep_largest, o.connectivity, o.min_island_area, o.max_hole_area) == (False, 8, 0, 0)
    assert Cleanup.parse(None) is None and Cleanup.parse(o) is o
    assert Cleanup.parse("largest") == Cleanup.uois() == Cleanup(True, 4) and Cleanup.parse("holes") == Cleanup.sam(300)
    assert Cleanup.sam(17).args() == (8, 0, 0, 17) and Cleanup(min_island_area=5, connectivity=4).args() == (4, 0, 5, 0)
    for kw in (dict(connectivity=6), dict(connectivity=True), dict(min_island_area=-1), dict(max_hole_area=-3), dict(max_hole_area=2.5),
               dict(min_island_area=2 ** 31), dict(keep_largest="yes"), dict(keep_largest=2), dict(connectivity=4.0), dict(connectivity=np.float32(8))):
        with pytest.raises(ValueError):
            Cleanup(**kw)
    assert Cleanup(np.bool_(True), np.int64(4), np.int32(7), np.int64(300)).args() == (4, 1, 7, 300)        # numpy integers are integers
    assert all(type(v) is int for v in Cleanup(np.bool_(True), np.int64(4), np.int32(7), np.int64(300)).args())
    for bad in ("islands", "", 4, True):
        with pytest.raises(ValueError):
            Cleanup.parse(bad)


def test_constructors_take_the_cleanup_keyword():
    from quber_amd.eval.refiner_model import MaskRefiner, MaskRefinerTTA
    from quber_amd.maskrefiner.predictor import MaskRefinerPredictor, RefinerModel
    for cls in (RefinerModel, MaskRefinerPredictor, MaskRefiner, MaskRefinerTTA):
        assert inspect.signature(cls.__init__).parameters["cleanup"].default is None, cls
    m = RefinerModel(None, {}, "cpu", tta=True, iterations=2)
    assert m.cleanup is None and (m.tta, m.iterations) == (True, 2)
    assert RefinerModel(None, {}, "cpu", cleanup="largest").cleanup == Cleanup.uois()
    assert RefinerModel(None, {}, "cpu", cleanup=Cleanup(max_hole_area=9)).cleanup.args() == (8, 0, 0, 9)
    with pytest.raises(ValueError):
        RefinerModel(None, {}, "cpu", cleanup="smallest")
    with pytest.raises(ValueError):
        MaskRefinerPredictor(None, device="cpu", state_dict={}, cleanup="smallest")
    with pytest.raises(ValueError):
        MaskRefiner(None, cleanup=3)
    with pytest.raises(ValueError):
        MaskRefinerTTA(None, cleanup="x")


# ---- the scenes of tests/test_gpu_cleanup.py ----
def serpentine(h, w, value=1, other=0):
    """A one-pixel-wide path over the whole frame: the even rows, joined alternately at their right and left ends."""
    a = np.full((h, w), other, np.int32)
    a[0::2] = value
    for k, y in enumerate(range(1, h, 2)):
        a[y, w - 1 if k % 2 == 0 else 0] = value
    return a


def scenes(h, w):
    """name -> (ids i32 [B,h,w], n_ids): the layouts at which the labelling can go wrong."""
    rng = np.random.default_rng(h * 1000 + w)
    s = {}
    # runs that end at the right edge and go on at the left of the next row / of the next frame's first row, and the pairs a flat
    # index joins by mistake: (y, w - 1) with (y, 0) [upper-right], (y, 0) with (y - 2, w - 1) [upper-left]
    a = np.zeros((3, h, w), np.int32)
    a[0, 4, w - 5:] = 1
    a[0, 5, :7] = 1
    a[0, h - 1, w - 4:] = 2
    a[1, 0, :9] = 2
    a[1, 0, w - 2:] = 2
    a[1, 9, :3] = 3
    a[1, 9, w - 4:] = 3
    a[1, 7, w - 6:] = 3
    a[2, 0, 0] = 1
    a[2, h - 1, w - 1] = 1
    a[2, h - 2, :w - 2] = 1
    a[1, h - 1, w - 3:] = 1
    s["row-and-frame-wrap"] = (a, 3)
    # the deepest parent chain, crossing every wave and block border; frame 1 the same path as void inside an instance; frame 2 upright
    a = np.zeros((3, h, w), np.int32)
    a[0] = serpentine(h, w)
    a[1] = serpentine(h, w, 0, 2)
    a[2, :, :h] = serpentine(w, h).T[:, :h] if h <= w else 0
    s["serpentine"] = (a, 2)
    cb = ((np.add.outer(np.arange(h), np.arange(w)) % 2) == 0).astype(np.int32)
    s["checkerboard"] = (np.stack([cb, 1 - cb, cb * 3]), 3)
    s["all-void"] = (np.zeros((2, h, w), np.int32), 4)
    s["all-one-instance"] = (np.full((2, h, w), 2, np.int32), 2)
    s["n-ids-0"] = (blocky(rng, (2, h, w), [0, 1, 2, -1, 255]), 0)
    a = blocky(rng, (3, h, w), [0, 0, 254, 253, 1, 255, 256, -1, 70000], cell=5, noise=0.05)
    s["id-254"] = (a, 254)
    s["random"] = (blocky(rng, (3, h, w), [0, 0, 1, 2, 3, 4, 5, 6, 7], cell=6, noise=0.05), 7)
    s["random-fine"] = (blocky(rng, (3, h, w), [0, 1, 2, 3], cell=2, noise=0.2), 3)
    s["hand-drawn-tiled"] = tiled_hand_scene(h, w)
    return s


def tiled_hand_scene(h, w):
    """Every hand-drawn case side by side in one (h, w) frame, one void column / row apart, clipped at the frame; three frames at
    different offsets (so that the drawings meet the wave borders differently) -> (ids [3,h,w], n_ids)."""
    a = np.zeros((3, h, w), np.int32)
    for f, (oy, ox) in enumerate(((0, 0), (3, 59), (h - 20, 1))):
        y, x = oy, ox
        for ids, n, o, want, rows in HAND.values():
            hh, ww = ids.shape[1:]
            if x + ww > w:
                y, x = y + 7, 0
            if y + hh > h:
                break
            a[f, y:y + hh, x:x + ww] = np.where((ids[0] >= 0) & (ids[0] <= 3), ids[0], 0)
            x += ww + 1
    return a, 3


def test_scenes_exercise_what_they_claim():
    for h, w in ((70, 131), (33, 64)):
        s = scenes(h, w)
        a, n = s["row-and-frame-wrap"]
        _, rep = cleanup_np(a, n, 8, True)
        assert rep[:, 1:, 0].tolist() == [[2, 1, 0], [1, 2, 3], [3, 0, 0]], rep[:, 1:, 0]
        a, n = s["serpentine"]
        for c in (4, 8):
            out, rep = cleanup_np(a, n, c, True, 0, 10 ** 6)
            assert rep[0, 1, 0] == 1 and rep[0, 1, 1] == 0 and (out[0] == 1).all() and (out[1] == 2).all() and rep[1, 0, 0] == 1
            assert rep[2, 1, 0] == 1 and rep[1, 2, 0] == h // 2              # the odd rows, each without one end pixel
        a, n = s["checkerboard"]
        _, r4 = cleanup_np(a, n, 4, True)
        _, r8 = cleanup_np(a, n, 8, True)
        assert r4[0, 1, 0] == (h * w + 1) // 2 and r4[0, 1, 3] == 1 and r8[0, 1, 0] == 1 and r8[0, 1, 1] == 0
        assert r4[2, 3, 3] == 1 and r4[1, 1, 3] == 1
        out, rep = cleanup_np(a, n, 4, False, 0, 2)
        assert (out[0] == 1).all() and rep[0, 0, 0] == h * w // 2
        a, n = s["id-254"]
        assert (a == 254).any() and cleanup_np(a, n, 8, True)[1][:, 254, 0].min() > 1
        assert cleanup_np(*s["n-ids-0"])[0].max() == 0
