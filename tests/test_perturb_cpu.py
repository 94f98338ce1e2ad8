"""CPU: the perturbed initial masks (INTEGRATION.md "Perturbed initial masks"; csrc/perturb.hip, quber_amd/perturb.py).

The contract in numpy (``perturb_np`` on the programs of ``quber_amd.perturb.perturb_program``: tests/test_gpu_perturb.py compares the
HIP path against it, masks and reports alike, exactly), the structuring elements pinned by hand-written arrays, the order of the random
draws against a transcription of the reference's code, hand-drawn cases, the ``Perturb`` validation, the ABI entry and the scenes the
GPU tests run.

The reference is ``perturb_seg`` (tools/ours/perturbation_utils.py:39-71).  Its ``compute_iou`` counts the non-zero pixels of
``seg * gt`` and ``seg + gt`` in uint8, which wraps.  With seg in {0, 255}: 255 * gt mod 256 = (256 - gt) mod 256 is non-zero exactly where
gt is, so the product is non-zero exactly where ``seg & g`` is (g = gt != 0); 255 + gt mod 256 = gt - 1 for gt >= 1, so the sum is
non-zero exactly where ``seg | g`` is - but for a set pixel of seg over gt == 1, where it wraps to 0.  The contract takes the sets,
``seg & g`` and ``seg | g``: the reference's counts for every mask without the value 1, its own 0 / 255 masks among them.

OpenCV is not installed here, so the agreement of ``structuring_element`` with ``cv2.getStructuringElement`` and of ``morph_np`` with
``cv2.dilate`` / ``cv2.erode`` on a numpy slice is ARGUED from OpenCV's source and documentation - the ellipse loop of
``cv::getStructuringElement`` (rows of ``[max(c - dx, 0), min(c + dx + 1, width))``, ``dx = cvRound(c * sqrt((r^2 - dy^2) / r^2))``), the
default anchor at ``(width / 2, height / 2)``, ``dst(x, y) = max / min over the set (x', y') of src(x + x' - anchor.x, y + y' - anchor.y)``,
and the default constant border, which reads as 0 for a dilation and as 1 for an erosion and which a sliced numpy array (an isolated
``cv::Mat`` without a parent) meets at the edge of the slice - and is not tested here."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from quber_amd import _lib
from quber_amd.perturb import COLUMNS, OPS_PER_ROUND, Perturb, perturb_program


# ---- the contract ----
def structuring_element(choice, size):
    """cv2.getStructuringElement for the reference's four choices: 1 a rectangle size x size; 2, 3, 4 ellipses of (width, height) =
    (size, size), (size, size // 2), (size // 2, size).  u8 [kh, kw].  Beyond what the reference draws: size is clamped to 1..15, a half
    size to >= 1, any other choice is a rectangle (what the kernel does with a malformed program)."""
    size = min(max(int(size), 1), 15)
    half = max(size // 2, 1)
    kw, kh = {2: (size, size), 3: (size, half), 4: (half, size)}.get(int(choice), (size, size))
    e = np.zeros((kh, kw), np.uint8)
    if int(choice) not in (2, 3, 4) or (kw == 1 and kh == 1):
        e[:] = 1
        return e
    r, c = kh // 2, kw // 2
    inv = 1.0 / (r * r) if r else 0.0
    for i in range(kh):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) * inv)))
            e[i, max(c - dx, 0):min(c + dx + 1, kw)] = 1
    return e


def morph_np(src, elem, dilate):
    """src bool [h, w] -> its dilation / erosion by `elem`, computed inside the array only: pixels beyond it count as 0 for a dilation,
    as 1 for an erosion.  dst(x, y) = max / min over the set (i, j) of src(x + j - kw // 2, y + i - kh // 2): no reflection."""
    h, w = src.shape
    kh, kw = elem.shape
    r, c = kh // 2, kw // 2
    p = np.full((h + 2 * kh, w + 2 * kw), not dilate, bool)
    p[kh:kh + h, kw:kw + w] = src
    out = np.full((h, w), not dilate, bool)
    for i, j in zip(*np.nonzero(elem)):
        win = p[kh + i - r:kh + i - r + h, kw + j - c:kw + j - c + w]
        out = (out | win) if dilate else (out & win)
    return out


def apply_op(seg, row):
    """One program row (lx, ly, lw, lh, clear, dilate, size, choice) on seg bool [h, w], in place.  The rectangle is clipped to the
    frame first (a program of perturb_program never needs it); the cleared pixel is skipped when it falls outside the frame."""
    h, w = seg.shape
    lx, ly, lw, lh, clear, dilate, size, choice = (int(v) for v in row)
    lx, lw = min(max(lx, 0), w), min(max(lw, 0), w)
    ly, lh = min(max(ly, 0), h), min(max(lh, 0), h)
    if clear:
        cx, cy = int((lx + lw) / 2), int((ly + lh) / 2)
        if cy < h and cx < w:
            seg[cy, cx] = False
    if lw > lx and lh > ly:
        seg[ly:lh, lx:lw] = morph_np(seg[ly:lh, lx:lw], structuring_element(choice, size), bool(dilate))


def perturb_np(gt, program, iou_target):
    """gt u8 [h, w], program int [n_ops, 8] -> (perturbed mask u8 [h, w] of 0 / 255, report i64 [4]: rounds executed, |seg & g|,
    |seg | g|, |seg| after the last executed round).  seg = gt > 127 is perturbed, the IoU is taken against g = gt != 0."""
    gt = np.asarray(gt)
    h, w = gt.shape
    seg, g = gt > 127, gt != 0
    rounds = 0
    if h > 2 and w > 2:
        program = np.asarray(program)
        assert len(program) % OPS_PER_ROUND == 0
        for k in range(0, len(program), OPS_PER_ROUND):
            for row in program[k:k + OPS_PER_ROUND]:
                apply_op(seg, row)
            rounds += 1
            iou = (np.count_nonzero(seg & g) + 1e-6) / (np.count_nonzero(seg | g) + 1e-6)
            if iou < iou_target:
                break
    return seg.astype(np.uint8) * 255, np.array([rounds, np.count_nonzero(seg & g), np.count_nonzero(seg | g), np.count_nonzero(seg)], np.int64)


def perturb_batch_np(masks, programs, targets):
    """masks u8 [B,N,H,W], programs [B,N,n_ops,8], targets [B,N] -> (u8 [B,N,H,W], i64 [B,N,4])."""
    B, N = masks.shape[:2]
    out, rep = np.empty_like(masks), np.empty((B, N, 4), np.int64)
    for b in range(B):
        for i in range(N):
            out[b, i], rep[b, i] = perturb_np(masks[b, i], programs[b, i], targets[b, i])
    return out, rep


# ---- the scenes of the GPU tests ----
def ellipse(h, w, cy=None, cx=None, ry=None, rx=None):
    """bool [h, w]: the axis-aligned ellipse of semi-axes h / 3, w / 4 around the frame's centre, unless told otherwise."""
    cy, cx = (h - 1) / 2 if cy is None else cy, (w - 1) / 2 if cx is None else cx
    ry, rx = h / 3 if ry is None else ry, w / 4 if rx is None else rx
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def scenes(h, w):
    """u8 [2, 3, h, w]: per frame an ellipse (255; in frame 1 off-centre, with a band of 128 - still seg - and a rim of 90 - g only),
    an empty mask, and a mask whose values are all <= 127 (g without seg: the perturbed mask stays empty)."""
    m = np.zeros((2, 3, h, w), np.uint8)
    m[0, 0] = ellipse(h, w) * 255
    e1, rim = ellipse(h, w, h * 0.45, w * 0.55), ellipse(h, w, h * 0.45, w * 0.55, h / 3 + 2, w / 4 + 2)
    m[1, 0] = np.where(e1, 255, np.where(rim, 90, 0))
    m[1, 0, h // 2:h // 2 + 2][e1[h // 2:h // 2 + 2]] = 128
    m[0, 2] = ellipse(h, w) * 127
    m[1, 2] = np.where(e1, 1, 0)
    m[1, 2, : h // 2][e1[: h // 2]] = 100
    return m


def test_scenes_are_what_the_gpu_tests_need():
    for h, w in ((33, 64), (70, 131), (9, 20)):
        m = scenes(h, w)
        assert m[:, 0].max() == 255 and (m[:, 0] > 127).reshape(2, -1).sum(1).min() > h * w // 8
        assert not m[:, 1].any()
        assert m[:, 2].any() and m[:, 2].max() <= 127
        assert set(np.unique(m[1, 0])) == {0, 90, 128, 255}
    # a target of 0.8 stops within a few rounds, one of 0.95 within 1-3, one of 0 never
    for h, w in ((33, 64), (70, 131)):
        gt = scenes(h, w)[0, 0]
        r8 = [int(perturb_np(gt, perturb_program(h, w, np.random.RandomState(s), rounds=30), 0.8)[1][0]) for s in range(6)]
        r95 = [int(perturb_np(gt, perturb_program(h, w, np.random.RandomState(s), rounds=30), 0.95)[1][0]) for s in range(6)]
        assert r8 == {(33, 64): [1, 2, 3, 5, 5, 3], (70, 131): [11, 6, 4, 5, 9, 9]}[(h, w)], r8       # (as first prototyped; pinned since)
        assert 1 <= min(r95) and max(r95) <= 3, r95
        assert all(a >= b for a, b in zip(r8, r95))
        out, rep = perturb_np(gt, perturb_program(h, w, np.random.RandomState(0), rounds=6), 0.0)
        assert rep[0] == 6 and rep[3] == np.count_nonzero(out)


# ---- structuring elements ----
def test_structuring_elements_pinned_by_hand():
    a = lambda rows: np.array(rows, np.uint8)
    np.testing.assert_array_equal(structuring_element(3, 5), a([[0, 0, 1, 0, 0], [1, 1, 1, 1, 1]]))
    np.testing.assert_array_equal(structuring_element(4, 4), a([[0, 1], [1, 1], [1, 1], [1, 1]]))
    e = structuring_element(2, 6)
    assert e.shape == (6, 6)
    np.testing.assert_array_equal(e[0], [0, 0, 0, 1, 0, 0])
    np.testing.assert_array_equal(e[1], [0, 1, 1, 1, 1, 1])
    np.testing.assert_array_equal(e[5], [0, 1, 1, 1, 1, 1])
    np.testing.assert_array_equal(structuring_element(1, 4), np.ones((4, 4), np.uint8))
    np.testing.assert_array_equal(structuring_element(2, 3), a([[0, 1, 0], [1, 1, 1], [0, 1, 0]]))
    np.testing.assert_array_equal(structuring_element(2, 5), a([[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]]))
    np.testing.assert_array_equal(structuring_element(3, 3), a([[0, 1, 0]]))             # height 3 // 2 = 1: r = 0, the centre column only
    np.testing.assert_array_equal(structuring_element(4, 3), a([[1], [1], [1]]))
    np.testing.assert_array_equal(structuring_element(3, 9), a([[0, 0, 0, 0, 1, 0, 0, 0, 0], [0, 1, 1, 1, 1, 1, 1, 1, 0], [1] * 9,
                                                                 [0, 1, 1, 1, 1, 1, 1, 1, 0]]))
    for choice in (1, 2, 3, 4):
        for size in range(1, 16):
            e = structuring_element(choice, size)
            kh, kw = e.shape
            assert e[kh // 2, kw // 2] == 1                                              # the anchor is set: an erosion never grows a mask
            for row in e:                                                                # every row is one contiguous run (the kernel relies on it)
                nz = np.flatnonzero(row)
                assert len(nz) == 0 or nz[-1] - nz[0] + 1 == len(nz)
    # what the reference never draws
    assert structuring_element(2, 40).shape == (15, 15) and structuring_element(1, 0).shape == (1, 1)
    assert structuring_element(3, 1).shape == (1, 1) and structuring_element(7, 5).all()


# ---- the order of the draws ----
def _reference_draws(seed, h, w, rounds):
    """perturb_seg's loop (perturbation_utils.py:51-66) with the pixel work left out: the same calls of the global numpy generator in
    the same order, through the same helper functions."""
    def get_random_structure(size):
        choice = np.random.randint(1, 5)
        return size, choice

    def random_dilate(min=3, max=10):
        size = np.random.randint(min, max)
        return get_random_structure(size)

    def random_erode(min=3, max=10):
        size = np.random.randint(min, max)
        return get_random_structure(size)

    np.random.seed(seed)
    rows = []
    for _ in range(rounds):
        for _ in range(4):
            lx, ly = np.random.randint(w), np.random.randint(h)
            lw, lh = np.random.randint(lx + 1, w + 1), np.random.randint(ly + 1, h + 1)
            clear = False
            if np.random.rand() < 0.25:
                clear = True
            if np.random.rand() < 0.5:
                size, choice = random_dilate()
                dilate = True
            else:
                size, choice = random_erode()
                dilate = False
            rows.append((lx, ly, lw, lh, clear, dilate, size, choice))
    return np.array(rows, np.int32)


def test_program_draws_in_the_reference_order():
    assert COLUMNS == ("lx", "ly", "lw", "lh", "clear", "dilate", "size", "choice") and OPS_PER_ROUND == 4
    for seed, (h, w) in enumerate(((33, 64), (70, 131), (480, 640), (3, 3))):
        state = np.random.get_state()
        want = _reference_draws(seed, h, w, 12)
        np.random.set_state(state)
        got = perturb_program(h, w, np.random.RandomState(seed), rounds=12)
        assert got.dtype == np.int32 and got.shape == (48, 8)
        np.testing.assert_array_equal(got, want)
        assert (got[:, 0] < got[:, 2]).all() and (got[:, 2] <= w).all() and (got[:, 1] < got[:, 3]).all() and (got[:, 3] <= h).all()
        assert set(np.unique(got[:, 6])) <= set(range(3, 10)) and set(np.unique(got[:, 7])) <= {1, 2, 3, 4}
    got = perturb_program(40, 50, np.random.RandomState(1), rounds=40, min_size=1, max_size=16)
    assert got[:, 6].min() == 1 and got[:, 6].max() == 15
    # the cleared pixel always lies inside its rectangle (the kernel applies it to the words it reads and never stores it)
    cx, cy = (got[:, 0] + got[:, 2]) // 2, (got[:, 1] + got[:, 3]) // 2
    assert (got[:, 0] <= cx).all() and (cx < got[:, 2]).all() and (got[:, 1] <= cy).all() and (cy < got[:, 3]).all()


# ---- hand-drawn cases ----
def _op(lx, ly, lw, lh, clear, dilate, size, choice):
    return (lx, ly, lw, lh, clear, dilate, size, choice)


NOP = _op(0, 0, 1, 1, 0, 1, 3, 1)          # dilates the 1 x 1 rectangle at a pixel the drawings leave empty: nothing changes


def _run(gt, ops, target=0.0):
    ops = list(ops) + [NOP] * (-len(ops) % OPS_PER_ROUND)
    return perturb_np(gt, np.array(ops, np.int32), target)


def test_one_pixel_wide_rectangle():
    gt = np.zeros((9, 9), np.uint8)
    gt[4, 3] = gt[4, 5] = 255
    out, rep = _run(gt, [_op(3, 1, 4, 8, 0, 1, 3, 1)])
    want = gt.copy()
    want[3:6, 3] = 255                                      # spreads along the column only; the neighbour column is not even read
    np.testing.assert_array_equal(out, want)
    assert rep.tolist() == [1, 2, 4, 4]
    out, _ = _run(want, [_op(3, 1, 4, 8, 0, 0, 3, 1)])     # the erosion sees 1 left and right of the rectangle: the column shrinks by its ends only
    np.testing.assert_array_equal(out, gt)


def test_rectangle_at_the_frame_corner():
    gt = np.zeros((8, 10), np.uint8)
    gt[5:, 6:] = 255
    out, _ = _run(gt, [_op(7, 6, 10, 8, 0, 0, 5, 1)])      # all ones inside, ones assumed outside (frame border included): unchanged
    np.testing.assert_array_equal(out, gt)
    out, _ = _run(gt, [_op(5, 4, 10, 8, 0, 0, 3, 1)])      # the zeros of row 4 and column 5 are INSIDE this rectangle: they eat one ring ...
    want = np.zeros_like(gt)
    want[6:, 7:] = 255                                      # ... but the frame's edge does not
    np.testing.assert_array_equal(out, want)
    gt2 = np.zeros((8, 10), np.uint8)
    gt2[7, 9] = 255
    out, _ = _run(gt2, [_op(8, 6, 10, 8, 0, 1, 9, 1)])     # a 9 x 9 dilation confined to the 2 x 2 corner
    want = np.zeros_like(gt2)
    want[6:, 8:] = 255
    np.testing.assert_array_equal(out, want)


def test_cleared_pixel_opens_a_hole_that_the_erosion_widens():
    gt = np.full((9, 9), 255, np.uint8)
    out, rep = _run(gt, [_op(0, 0, 9, 9, 1, 0, 3, 1)])
    want = gt.copy()
    want[3:6, 3:6] = 0                                      # (int((0 + 9) / 2), int((0 + 9) / 2)) = (4, 4), widened by the 3 x 3 erosion
    np.testing.assert_array_equal(out, want)
    assert rep.tolist() == [1, 72, 81, 72]
    out, _ = _run(gt, [_op(0, 0, 9, 9, 1, 1, 3, 1)])       # a dilation closes it again
    np.testing.assert_array_equal(out, gt)
    out, _ = _run(gt, [_op(2, 2, 5, 4, 1, 1, 3, 4)])       # cleared at (3, 3); the 1 x 3 column element refills it from above ... there is no
    np.testing.assert_array_equal(out, gt)                  # row below inside the rectangle: the row above is enough


def test_even_sizes_shift_as_the_formula_says():
    gt = np.zeros((12, 12), np.uint8)
    gt[5, 5] = 255
    out, _ = _run(gt, [_op(0, 0, 12, 12, 0, 1, 4, 1)])     # dst(x) = max src(x + j - 2), j = 0..3: the pixel spreads 1 left / up, 2 right / down
    want = np.zeros_like(gt)
    want[4:8, 4:8] = 255
    np.testing.assert_array_equal(out, want)
    out, _ = _run(want, [_op(0, 0, 12, 12, 0, 0, 4, 1)])   # min src(x - 2 .. x + 1): x - 2 >= 4 and x + 1 <= 7
    want2 = np.zeros_like(gt)
    want2[6, 6] = 255
    np.testing.assert_array_equal(out, want2)
    out, _ = _run(gt, [_op(0, 0, 12, 12, 0, 1, 4, 4)])     # [[0,1],[1,1],[1,1],[1,1]]: anchor (1, 2)
    want3 = np.zeros_like(gt)
    want3[4:8, 5] = 255                                     # column j = 1 (dx = 0), rows i - 2 = -2 .. 1 -> y = 5 - dy = 7 .. 4
    want3[4:7, 6] = 255                                     # column j = 0 (dx = -1 -> x = 6), rows i = 1 .. 3 -> y = 6 .. 4
    np.testing.assert_array_equal(out, want3)


def test_threshold_values_seg_and_g():
    gt = np.zeros((4, 6), np.uint8)
    gt[1, 1:5] = (1, 127, 128, 255)
    out, rep = _run(gt, [])                                  # no operation at all: no round
    assert rep.tolist() == [0, 2, 4, 2]
    out, rep = _run(gt, [NOP])
    np.testing.assert_array_equal(out, np.where(gt > 127, 255, 0))
    assert rep.tolist() == [1, 2, 4, 2]                      # seg = {128, 255}, g = all four
    # iou = 2 / 4: a target above it stops after round 1, one below it never
    prog = np.array([NOP] * 12, np.int32)
    assert perturb_np(gt, prog, 0.6)[1][0] == 1 and perturb_np(gt, prog, 0.5)[1][0] == 3
    # an empty seg against a non-empty g: iou = 1e-6 / (|g| + 1e-6); both empty: iou = 1, never below a target <= 1
    low = np.where(gt > 0, 100, 0).astype(np.uint8)
    assert perturb_np(low, prog, 0.3)[1].tolist() == [1, 0, 4, 0] and perturb_np(low, prog, 0.0)[1].tolist() == [3, 0, 4, 0]
    assert perturb_np(np.zeros_like(gt), prog, 1.0)[1].tolist() == [3, 0, 0, 0]


def test_frames_of_two_rows_or_columns_come_back_thresholded():
    prog = perturb_program(5, 5, np.random.RandomState(0), rounds=2)
    for shape in ((2, 7), (7, 2), (1, 1)):
        gt = np.full(shape, 200, np.uint8)
        gt[0, 0] = 90
        out, rep = perturb_np(gt, prog, 0.9)
        np.testing.assert_array_equal(out, np.where(gt > 127, 255, 0))
        assert rep.tolist() == [0, gt.size - 1, gt.size, gt.size - 1]


def test_malformed_programs_are_clipped():
    gt = scenes(9, 20)[0, 0]
    bad = np.array([_op(-5, -3, 400, 300, 1, 1, 40, 2), _op(15, 7, 99, 99, 0, 0, 0, 9), _op(30, 30, 10, 10, 1, 1, 5, 1), _op(12, 4, 6, 4, 1, 0, -4, 3)], np.int32)
    # the same, well formed: the whole frame with the largest ellipse; a 1 x 1 erosion; an empty rectangle whose cleared pixel lies
    # outside the frame (skipped); an empty rectangle whose cleared pixel (4, 9) lies inside (cleared)
    good = np.array([_op(0, 0, 20, 9, 1, 1, 15, 2), _op(15, 7, 20, 9, 0, 0, 1, 1), _op(20, 9, 10, 9, 0, 1, 5, 1), _op(9, 4, 10, 5, 1, 0, 1, 1)], np.int32)
    assert gt[4, 9] == 255
    a, ra = perturb_np(gt, bad, 0.0)
    b, rb = perturb_np(gt, good, 0.0)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ra, rb)
    assert a[4, 9] == 0 and a[4, 8] == 255                   # the one pixel the last operation cleared


# ---- the word-level form the kernel computes in ----
def _perturb_words(gt, program, iou_target):
    """perturb_np restated the way csrc/perturb.hip computes: bit planes of 32-bit words, per word a 96-bit window shifted once and
    folded by doubling, an erosion as the dilation of the complement, the cleared pixel applied to the words as they are read."""
    h, w = gt.shape
    wpr = (w + 31) // 32
    pack = lambda m: [[sum(int(m[y, x]) << (x - 32 * j) for x in range(32 * j, min(32 * j + 32, w))) for j in range(wpr)] for y in range(h)]
    seg, g = pack(gt > 127), pack(gt != 0)
    M32 = 0xFFFFFFFF
    count = lambda: (sum(bin(a & b).count("1") for ra, rb in zip(seg, g) for a, b in zip(ra, rb)),
                     sum(bin(a | b).count("1") for ra, rb in zip(seg, g) for a, b in zip(ra, rb)), sum(bin(a).count("1") for ra in seg for a in ra))

    def colmask(wx, lx, lw):
        lo, hi = max(lx - 32 * wx, 0), min(lw - 32 * wx, 32)
        return 0 if hi <= lo else ((1 << hi) - 1) & ~((1 << lo) - 1) & M32

    rounds = 0
    if h > 2 and w > 2:
        for k, row in enumerate(np.asarray(program).tolist()):
            lx, ly, lw, lh = min(max(row[0], 0), w), min(max(row[1], 0), h), min(max(row[2], 0), w), min(max(row[3], 0), h)
            clear, dilate = row[4] != 0, row[5] != 0
            elem = structuring_element(row[7], row[6])
            kh, kw = elem.shape
            r, c, cx, cy = kh // 2, kw // 2, (lx + lw) // 2, (ly + lh) // 2
            cbit = 1 << (cx & 31) if clear else 0
            if lw > lx and lh > ly:
                tmp = {}
                for y in range(ly, lh):
                    for wx in range(lx >> 5, ((lw - 1) >> 5) + 1):
                        ms = [colmask(wx + d, lx, lw) for d in (-1, 0, 1)]
                        acc = 0
                        for i in range(kh):
                            nz = np.flatnonzero(elem[i])
                            ys = y + i - r
                            if len(nz) == 0 or ys < ly or ys >= lh:
                                continue
                            a, b = int(nz[0]), int(nz[-1]) + 1
                            v = [seg[ys][wx + d] if ms[d + 1] else 0 for d in (-1, 0, 1)]
                            if ys == cy:
                                v = [x & ~cbit if (cx >> 5) == wx + d else x for d, x in zip((-1, 0, 1), v)]
                            if not dilate:
                                v = [~x & M32 for x in v]
                            v = [x & m for x, m in zip(v, ms)]
                            s0, ln = 32 + a - c, b - a
                            assert 25 <= s0 <= 32 and 1 <= ln <= 15
                            win = (((v[1] << 32 | v[0]) >> s0) | (v[2] << (64 - s0))) & 0xFFFFFFFFFFFFFFFF
                            s = 1
                            while 2 * s <= ln:
                                win |= win >> s
                                s *= 2
                            if ln > s:
                                win |= win >> (ln - s)
                            acc |= win & M32
                        tmp[(y, wx)] = (seg[y][wx] & ~ms[1]) | ((acc if dilate else ~acc & M32) & ms[1])
                for (y, wx), v in tmp.items():
                    seg[y][wx] = v
            elif cbit and cy < h and cx < w:
                seg[cy][cx >> 5] &= ~cbit
            if (k + 1) % OPS_PER_ROUND == 0:
                rounds += 1
                ci, cu, _ = count()
                if (ci + 1e-6) / (cu + 1e-6) < iou_target:
                    break
    out = np.array([[(seg[y][x >> 5] >> (x & 31)) & 1 for x in range(w)] for y in range(h)], np.uint8) * 255
    return out, np.array((rounds,) + count(), np.int64)


@pytest.mark.parametrize("h,w", [(33, 64), (9, 20), (20, 131)], ids=["33x64", "9x20", "20x131"])
def test_word_level_form_equals_the_contract(h, w):
    gt = scenes(h, w)[1, 0]
    for seed, target in ((0, 0.8), (1, 0.0)):
        prog = perturb_program(h, w, np.random.RandomState(seed), rounds=3, min_size=1, max_size=16)
        want, rep = perturb_np(gt, prog, target)
        got, got_rep = _perturb_words(gt, prog, target)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_rep, rep)


# ---- the public constructor ----
def test_perturb_validation():
    p = Perturb(0.8, seed=3)
    assert (p.rounds, p.min_size, p.max_size, p.n_ops) == (250, 3, 10, 1000)
    assert p.targets(2, 3).shape == (2, 3) and p.targets(2, 3).dtype == np.float64 and (p.targets(2, 3) == 0.8).all()
    assert p.mask_seeds(2, 3).tolist() == [[3, 4, 5], [6, 7, 8]]
    assert p == Perturb(0.8, seed=3) and p != Perturb(0.8, seed=4) and hash(p) == hash(Perturb(np.float64(0.8), seed=np.int64(3)))
    assert "0.8" in repr(p)
    q = Perturb([0.9, 0.8, 0.0], rounds=2, seeds=[[5, 5, 7]])
    assert q.targets(2, 3).tolist() == [[0.9, 0.8, 0.0]] * 2 and q.mask_seeds(2, 3).tolist() == [[5, 5, 7]] * 2
    progs = q.programs(2, 3, 12, 17)
    assert progs.shape == (2, 3, 8, 8) and progs.dtype == np.int32 and not progs.flags.writeable
    np.testing.assert_array_equal(progs[0, 0], progs[1, 1])
    np.testing.assert_array_equal(progs[0, 2], perturb_program(12, 17, np.random.RandomState(7), rounds=2))
    assert q.programs(2, 3, 12, 17) is progs                             # drawn once
    np.testing.assert_array_equal(Perturb(0.5, seed=2, rounds=1).programs(1, 2, 9, 9)[0, 1], perturb_program(9, 9, np.random.RandomState(3), rounds=1))
    with pytest.raises(ValueError):
        q.targets(2, 4)
    for bad in (dict(iou_target=1.5), dict(iou_target=-0.1), dict(iou_target=float("nan")), dict(iou_target="0.8"), dict(iou_target=True),
                dict(iou_target=np.zeros((2, 2, 2))), dict(iou_target=[]),
                dict(iou_target=0.8, seed=1.0), dict(iou_target=0.8, seed=-1), dict(iou_target=0.8, seed=True), dict(iou_target=0.8, rounds=0),
                dict(iou_target=0.8, rounds=2.0), dict(iou_target=0.8, min_size=0), dict(iou_target=0.8, min_size=5, max_size=5),
                dict(iou_target=0.8, max_size=17), dict(iou_target=0.8, seeds=[0.5]), dict(iou_target=0.8, seeds=[-1]), dict(iou_target=0.8, seeds=[])):
        with pytest.raises(ValueError):
            Perturb(**bad)


# ---- the ABI entry ----
def test_abi_entry_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "quber_hip.h")).read()
    m = re.search(r"\bint\s+quber_perturb_masks\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert m, "quber_perturb_masks is not declared in include/quber_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    res, argtypes = _lib.SIGNATURES["quber_perturb_masks"]
    assert res is ctypes.c_int and len(argtypes) == len(args) == 12
    for a, t in zip(args, argtypes):
        assert (("*" in a) and t is ctypes.c_void_p) or (("int32_t" in a) and t is ctypes.c_int32), (a, t)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "quber_perturb_masks")
    src = open(os.path.join(ROOT, "quber_amd", "csrc", "Makefile")).read()
    assert "perturb.hip" in src
