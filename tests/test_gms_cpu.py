"""CPU: the contract of the Gaussian mean shift that turns UOIS-Net-3D's centre votes into initial masks, and of the initial mask
processing (IMP) behind it (csrc/gms.hip, Engine.gms, MaskRefinerPredictor(cluster=GaussianMeanShift())), stated in numpy, and what can
be checked of the feature without a GPU.

The reference (uois/src/segmentation.py:129-187 DSNWrapper.cluster, uois/src/cluster.py GaussianMeanShift, segmentation.py:425-491
process_initial_masks): of the foreground pixels' votes every subsample-th seeds and climbs; ``select_smart_seeds`` draws num_seeds of
them with probability proportional to the distance from the seeds already drawn, ``seed_hill_climbing`` moves them max_iters times to
the Gaussian-weighted mean of the points, ``connected_components`` gives seeds within epsilon of one another the same label, every
foreground pixel takes the label of its nearest seed, clusters under min_pixels are dropped; then every mask is opened and closed with
OpenCV's 9 x 9 ellipse, in ascending id on the current map, and cut down to its largest 4-connected component.  ``gms_np`` / ``imp_np``
restate this in the arithmetic the device reproduces; tests/golden/gms_*.npz (tools/gen_gms_golden.py) were recorded from the
reference's own functions.

Where the contract pins what the reference leaves open:
  * dist(a, b) = sqrt((dx dx + dy dy) + dz dz) in float32, every operation rounded separately (torch.norm leaves the order open).
  * the random choice of the seeds is an argument: the first seed, and a 32-bit draw r_k per further seed, which picks the first point
    whose inclusive prefix sum of q = min(floor(float64(mind) 2^20), 2^31 - 1) exceeds floor(r_k total / 2^32) - torch.multinomial on
    the distances quantised to 2^-20, in integers.  S = min(num_seeds, n_sub) seeds: the reference leaves the others uninitialised.
  * the climb is stated in float64 on the float32 inputs; the device computes it in float32 and is held to 4 x the error of the
    reference's float32 formula (tests/test_gpu_gms.py).  A seed whose weights sum to 0 keeps its position; the reference divides 0 by 0.
  * clusters are numbered 1..count (the reference's OBJECTS_LABEL = 2 is an offset of its own network's label space).
"""
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from conftest import ROOT
from quber_amd.gms import IMP, MAX_SEEDS, GaussianMeanShift, imp_plane_bytes

GOLDEN = os.path.join(ROOT, "tests", "golden")
F32 = np.float32


# ---- the contract: clustering ----
def dist_np(A, Bm):
    """A f32 [m,3], Bm f32 [k,3] -> f32 [m,k]: sqrt((dx dx + dy dy) + dz dz), every operation rounded to float32."""
    A, Bm = np.asarray(A, F32), np.asarray(Bm, F32)
    dx, dy, dz = (A[:, None, c] - Bm[None, :, c] for c in range(3))
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def compact_np(votes, fg, subsample):
    """votes f32 [3,H,W], fg [H,W] -> (P f32 [n,3]: the foreground votes in row-major order, Xs = P[::subsample])."""
    P = np.ascontiguousarray(np.asarray(votes, F32).reshape(3, -1).T[np.asarray(fg).reshape(-1) != 0])
    return P, P[::subsample]


def quantise(mind):
    return np.minimum(np.floor(np.asarray(mind, np.float64) * 2.0 ** 20), 2.0 ** 31 - 1).astype(np.int64)


def seeds_np(Xs, first, r, num_seeds):
    """Xs f32 [n_sub,3], r: 32-bit draws (r[k] picks seed k; r[0] is not read) -> i32 [S], S = min(num_seeds, n_sub)."""
    S = min(num_seeds, len(Xs))
    idx = np.empty(S, np.int32)
    if S == 0:
        return idx
    idx[0] = min(max(int(first), 0), len(Xs) - 1)
    mind = dist_np(Xs, Xs[idx[0]:idx[0] + 1])[:, 0]
    for k in range(1, S):
        q = quantise(mind)
        total = int(q.sum())
        t = (int(r[k]) * total) >> 32
        idx[k] = int(np.searchsorted(np.cumsum(q), t, side="right")) if total > 0 else 0      # the first p with prefix[p] > t
        mind = np.minimum(mind, dist_np(Xs, Xs[idx[k]:idx[k] + 1])[:, 0])
    return idx


def climb_np(Xs, Z, sigma, iters):
    """float64: iters times W = exp(-0.5 / sigma^2 |Z - Xs|^2), Z = (W Xs) / sum W; a seed whose weights sum to 0 stays."""
    X64, Z = np.asarray(Xs, np.float64), np.array(Z, np.float64)
    for _ in range(iters):
        if not len(X64) or not len(Z):
            break
        W = np.exp(-0.5 / sigma ** 2 * sum((Z[:, None, c] - X64[None, :, c]) ** 2 for c in range(3)))
        sw = W.sum(1, keepdims=True)
        Z = np.where(sw > 0, (W @ X64) / np.where(sw > 0, sw, 1.0), Z)
    return Z


def link_np(Z, epsilon):
    """Z f32 [S,3] -> i32 [S]: connected_components (cluster.py:60-90) as written."""
    Z = np.asarray(Z, F32).reshape(-1, 3)
    S = Z.shape[0]
    near = dist_np(Z, Z) <= F32(epsilon)
    labels = -np.ones(S, np.int32)
    K = 0
    for i in range(S):
        if labels[i] != -1:
            continue
        comp = near[:, i]
        seen = labels[comp]
        if len(np.unique(seen)) > 1:
            vals, counts = np.unique(seen[seen != -1], return_counts=True)
            label = vals[np.argmax(counts)]                  # torch.mode: the smallest label among equal counts
        else:
            label = K
            K += 1
        labels[comp] = label
    return labels


def assign_np(P, Z, seed_labels):
    """-> (nearest i32 [n]: the first index of the minimum dist, labels i32 [n])."""
    if not len(P) or not len(Z):
        return np.zeros(len(P), np.int32), -np.ones(len(P), np.int32)
    nearest = np.concatenate([np.argmin(dist_np(P[i:i + 16384], Z), axis=1) for i in range(0, len(P), 16384)]).astype(np.int32)
    return nearest, np.asarray(seed_labels, np.int32)[nearest]


def filter_np(labels, Z, seed_labels, min_pixels, max_masks=None):
    """labels i32 [n] (assign_np) -> (ids i32 [n]: 1..count, 0 dropped; centers f32 [count,3]: the mean of the climbed seeds that carry
    the label, a float32 sum in seed order divided by their number; report i32 [4]: count, clusters found, dropped by min_pixels,
    truncated).  Survivors are numbered in ascending label order; those behind max_masks are dropped and reported as truncated."""
    labels, seed_labels, Z = np.asarray(labels, np.int32), np.asarray(seed_labels, np.int32), np.asarray(Z, F32).reshape(-1, 3)
    K = int(seed_labels.max()) + 1 if len(seed_labels) else 0
    keep = [l for l in range(K) if (labels == l).sum() >= min_pixels]
    dropped = K - len(keep)
    truncated = int(max_masks is not None and len(keep) > max_masks)
    if truncated:
        keep = keep[:max_masks]
    ids = np.zeros_like(labels)
    centers = np.zeros((len(keep), 3), F32)
    for k, l in enumerate(keep):
        ids[labels == l] = k + 1
        acc = np.zeros(3, F32)
        for s in np.flatnonzero(seed_labels == l):
            acc = acc + Z[s]
        centers[k] = acc / F32((seed_labels == l).sum())
    return ids, centers, np.array([len(keep), K, dropped, truncated], np.int32)


# ---- the contract: IMP ----
def ellipse(k):
    """cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)), u8 [k,k]: the formula tests/test_perturb_cpu.py: structuring_element argues
    from OpenCV's source (row dy of a circle of radius r = k // 2 is rint(r sqrt((r^2 - dy^2) / r^2)) wide to either side)."""
    r = k // 2
    e = np.zeros((k, k), np.uint8)
    inv = 1.0 / (r * r) if r else 0.0
    for i in range(k):
        dy = i - r
        dx = int(np.rint(r * np.sqrt((r * r - dy * dy) * inv)))
        e[i, max(r - dx, 0):min(r + dx + 1, k)] = 1
    return e


def morph_np(mask, elem, erode):
    """mask bool [h,w] -> its erosion (beyond the frame reads as 1) or dilation (as 0) by elem: OpenCV's default constant border."""
    h, w = mask.shape
    r = elem.shape[0] // 2
    pad = np.pad(mask.astype(bool), r, constant_values=bool(erode))
    out = np.full((h, w), bool(erode))
    for i, j in zip(*np.nonzero(elem)):
        win = pad[i:i + h, j:j + w]
        out = (out & win) if erode else (out | win)
    return out


def open_close_np(mask, elem):
    opened = morph_np(morph_np(mask, elem, True), elem, False)
    return morph_np(morph_np(opened, elem, False), elem, True)


def largest_component_np(mask):
    """The largest 4-connected component of mask, the one whose first pixel comes first in raster order among equals; all False if
    mask is.  A flood fill of its own, so that scipy stays the thing it is tested against."""
    h, w = mask.shape
    seen = np.zeros((h, w), bool)
    best, best_n = None, 0
    for y0, x0 in zip(*np.nonzero(mask)):
        if seen[y0, x0]:
            continue
        stack, comp = [(y0, x0)], []
        seen[y0, x0] = True
        while stack:
            y, x = stack.pop()
            comp.append((y, x))
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < h and 0 <= xx < w and mask[yy, xx] and not seen[yy, xx]:
                    seen[yy, xx] = True
                    stack.append((yy, xx))
        if len(comp) > best_n:
            best, best_n = comp, len(comp)
    out = np.zeros((h, w), bool)
    if best:
        out[tuple(np.array(best).T)] = True
    return out


def imp_np(ids, n_ids, ksize=9, largest=True):
    """ids i32 [h,w] (0, 1..n_ids; anything else counts as 0) -> (ids after the IMP, renumbered 1..count; report i32 [2]: count, ids
    that were present and are empty now; keep: the old ids that stay, ascending).  Sequential, as the reference loops: for o ascending
    on the CURRENT map, mask = ids == o, ids[mask] = 0, ids[open_close(mask)] = o; then the largest component per id."""
    ids = np.array(ids, np.int32)
    ids[(ids < 0) | (ids > n_ids)] = 0
    before = [o for o in range(1, n_ids + 1) if (ids == o).any()]
    elem = ellipse(ksize)
    for o in before:                                         # (an absent id is a no-op: the opening of an empty mask is empty)
        mask = ids == o
        res = open_close_np(mask, elem)
        ids[mask] = 0
        ids[res] = o
    if largest:
        for o in range(1, n_ids + 1):
            mask = ids == o
            ids[mask] = 0
            ids[largest_component_np(mask)] = o
    keep = [o for o in range(1, n_ids + 1) if (ids == o).any()]
    out = np.zeros_like(ids)
    for k, o in enumerate(keep):
        out[ids == o] = k + 1
    return out, np.array([len(keep), len(before) - len(keep)], np.int32), keep


# ---- the chain ----
def gms_np(votes, fg, first, r, g, max_masks=None):
    """One frame under g (a GaussianMeanShift).  -> dict: info (n, n_sub, S), indices i32 [S], seeds f32 [S,3] (the climbed seeds,
    float64 rounded once), seed_labels i32 [S], raw_ids i32 [H,W] (before the IMP), ids i32 [H,W], centers f32 [count,3], report i32 [6]
    = count, clusters found, dropped by min_pixels, truncated, emptied by the IMP, fg pixels."""
    fg = np.asarray(fg) != 0
    h, w = fg.shape
    P, Xs = compact_np(votes, fg, g.subsample)
    idx = seeds_np(Xs, first, r, g.num_seeds)
    Z = climb_np(Xs, Xs[idx], g.sigma, g.iters).astype(F32).reshape(-1, 3)
    sl = link_np(Z, g.epsilon)
    nearest, lab = assign_np(P, Z, sl)
    pid, centers, rep = filter_np(lab, Z, sl, g.min_pixels, max_masks)
    raw = np.zeros(h * w, np.int32)
    raw[fg.reshape(-1)] = pid
    raw = raw.reshape(h, w)
    ids, emptied = raw, 0
    if g.imp is not None:
        ids, irep, keep = imp_np(raw, int(rep[0]), g.imp.ksize, g.imp.largest)
        centers, emptied = centers[[o - 1 for o in keep]], int(irep[1])
    count = int(ids.max()) if ids.size else 0
    report = np.array([count, rep[1], rep[2], rep[3], emptied, len(P)], np.int32)
    return {"info": np.array([len(P), len(Xs), len(idx)], np.int32), "indices": idx, "seeds": Z, "seed_labels": sl, "nearest": nearest,
            "labels": lab, "raw_ids": raw, "ids": ids, "centers": centers.reshape(-1, 3), "report": report}


def decidable(P, Z, seed_labels, epsilon, margin=1e-4):
    """What the chain tests require of an input before they ask for equal label maps: every seed-to-seed distance is more than `margin`
    away from epsilon, and for every pixel the nearest seed of any other cluster is more than `margin` farther than that of its own."""
    Z64, P64 = np.asarray(Z, np.float64), np.asarray(P, np.float64)
    if not len(Z64) or not len(P64):
        return True
    dz = np.sqrt(((Z64[:, None] - Z64[None]) ** 2).sum(-1))
    if np.abs(dz - epsilon).min() <= margin:
        return False
    labs = np.unique(seed_labels)
    for i in range(0, len(P64), 16384):
        d = np.sqrt(sum((P64[i:i + 16384, None, c] - Z64[None, :, c]) ** 2 for c in range(3)))
        per = np.stack([d[:, seed_labels == l].min(axis=1) for l in labs], axis=1)
        per.sort(axis=1)
        if per.shape[1] > 1 and (per[:, 1] - per[:, 0]).min() <= margin:
            return False
    return True


def same_partition(a, b):
    """Two label maps describe the same partition with label 0 on the same pixels."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    pairs = {(int(x), int(y)) for x, y in zip(a, b)}
    return len({x for x, _ in pairs}) == len(pairs) == len({y for _, y in pairs}) and np.array_equal(a == 0, b == 0)


# ---- inputs ----
def vote_scene(h, w, k, seed, noise=0.003, stray=0, gap=2):
    """(votes f32 [3,h,w], fg u8 [h,w], which i32 [h,w]: 0 background, 1..k): k objects in vertical stripes separated by `gap` background
    columns; a foreground pixel votes for its object's centre (0.25 m apart) plus Gaussian noise; `stray` foreground pixels in the gaps
    vote for places of their own, far from everything.  Background pixels carry votes too (the table's): they must be ignored."""
    rng = np.random.RandomState(seed)
    centres = np.array([[0.25 * j - 0.3, 0.1 * (j % 2) - 0.05, 0.8 + 0.05 * j] for j in range(k)])
    edges = np.linspace(0, w, k + 1).astype(int)
    which = np.zeros((h, w), np.int32)
    for j in range(k):
        which[1:h - 1, edges[j] + gap:edges[j + 1]] = j + 1
    votes = np.array([0.0, 0.3, 1.2])[:, None, None] + 0.2 * rng.rand(3, h, w)
    on = which > 0
    votes[:, on] = centres[which[on] - 1].T + noise * rng.randn(3, int(on.sum()))
    fg = on.astype(np.uint8)
    cols = [c for j in range(k) for c in range(edges[j], edges[j] + gap)]
    for i in range(stray):
        y, x = 1 + (7 * i) % (h - 2), cols[i % len(cols)]
        fg[y, x] = 1
        votes[:, y, x] = [2.0 + 0.5 * i, -1.0, 3.0]
    return np.ascontiguousarray(votes.astype(F32)), fg, which


def voronoi_map(h, w, k, seed, noise=0.03, holes=4):
    """i32 [h,w] in 0..k: the Voronoi cells of k random sites (touching regions), `noise` of the pixels re-drawn from 0..k, and a few
    3 x 3 holes: what the IMP is for."""
    rng = np.random.RandomState(seed)
    sites = np.stack([rng.randint(0, h, k), rng.randint(0, w, k)], 1)
    yy, xx = np.mgrid[:h, :w]
    ids = (np.argmin((yy[..., None] - sites[:, 0]) ** 2 + (xx[..., None] - sites[:, 1]) ** 2, axis=-1) + 1).astype(np.int32)
    flip = rng.rand(h, w) < noise
    ids[flip] = rng.randint(0, k + 1, int(flip.sum()))
    for _ in range(holes):
        y, x = rng.randint(0, h - 3), rng.randint(0, w - 3)
        ids[y:y + 3, x:x + 3] = 0
    return ids


def chain_cases():
    """name -> (Z f32 [6,3], the seed labels connected_components gives them): seeds on a line whose epsilon balls are NOT transitive, so
    that the labelling meets seeds that already carry labels - the mode branch, which collapsed seeds never reach.  epsilon = 0.05; the
    seeds sit at the given x (metres), y = 0, z = 0.5, and no distance is within 5e-3 of epsilon.  Named k, o, j, m1, m2, i: k's ball
    holds j but not i; o's ball holds m1 (and m2); i, the last seed, is in nobody's ball and its own holds j and m1 (and m2)."""
    def seeds(*xs):
        Z = np.zeros((len(xs), 3), F32)
        Z[:, 0], Z[:, 2] = xs, 0.5
        return Z
    return {
        # i meets j (label 0) and m1, m2 (label 1): the mode, 1, wins over the smaller label and j is re-labelled
        "chain_mode": (seeds(0.0, 0.16, 0.04, 0.12, 0.124, 0.08), [0, 1, 1, 1, 1, 1]),
        # m2 out of i's reach: one seed of each label, equal counts -> the smallest label, 0; m1 is re-labelled
        "chain_tie": (seeds(0.0, 0.16, 0.04, 0.12, 0.14, 0.08), [0, 1, 0, 0, 1, 0]),
        # the same tie with o before k, so that the seed i meets FIRST (j, index 2) carries the larger label: still the smallest label
        "chain_tie_order": (seeds(0.16, 0.0, 0.04, 0.12, 0.14, 0.08), [0, 1, 0, 0, 0, 0]),
    }


def small_options(**kw):
    """The reference's settings scaled to frames of a few hundred foreground pixels."""
    return GaussianMeanShift(**dict(dict(num_seeds=40, min_pixels=20, imp=None), **kw))


def _golden(name):
    return np.load(os.path.join(GOLDEN, name))


# ---- tests ----
def test_contract_properties_on_a_scene():
    votes, fg, which = vote_scene(37, 53, 4, seed=3, stray=3)
    g = small_options()
    first, r = GaussianMeanShift(num_seeds=40, seed=5).draws([g.n_sub(int(fg.sum()))])
    out = gms_np(votes, fg, first[0], r[0], g)
    P, Xs = compact_np(votes, fg, g.subsample)
    n = int(fg.sum())
    assert n % g.subsample != 0 and out["info"].tolist() == [n, -(-n // 5), 40] and len(Xs) == -(-n // 5)
    assert decidable(P, out["seeds"], out["seed_labels"], g.epsilon)
    # the four objects, and the strays that were drawn as seeds: clusters of one pixel, dropped
    assert out["report"][0] == 4 and out["report"][1] > 4 and out["report"][2] == out["report"][1] - 4 and out["report"][5] == n
    assert same_partition(out["ids"], np.where(out["ids"] > 0, which, 0)) and (out["ids"][which > 0] > 0).all()
    assert not out["ids"][fg == 0].any()
    true = np.array([[0.25 * j - 0.3, 0.1 * (j % 2) - 0.05, 0.8 + 0.05 * j] for j in range(4)])
    obj = [int(which[out["ids"] == k + 1][0]) - 1 for k in range(4)]       # the clusters are numbered by seed label, not by stripe
    assert sorted(obj) == [0, 1, 2, 3] and np.abs(out["centers"] - true[obj]).max() < 2e-3
    assert gms_np(votes, fg, first[0], r[0], g, max_masks=2)["report"].tolist()[:4] == [2, out["report"][1], out["report"][2], 1]


def test_seed_selection():
    votes, fg, _ = vote_scene(24, 32, 3, seed=1)
    _, Xs = compact_np(votes, fg, 5)
    r = np.random.RandomState(9).randint(0, 2 ** 32, size=12, dtype=np.uint64).astype(np.uint32)
    idx = seeds_np(Xs, 7, r, 12)
    assert idx.tolist() == LITERAL_SEEDS, idx.tolist()
    # a point already chosen has q = 0: no threshold selects it again while total > 0
    assert len(set(idx.tolist())) == 12
    Y = np.repeat(Xs[:3], [4, 1, 1], axis=0)                 # duplicates of a chosen point have q = 0 too and are skipped
    for rk in (0, 1, 2 ** 31, 2 ** 32 - 1):
        got = seeds_np(Y, 0, np.array([0, rk, rk], np.uint32), 3)
        assert got[1] in (4, 5) and got[2] in (4, 5) and got[1] != got[2], (rk, got)
    # the smallest and the largest draw pick the first and the last point with q > 0
    mind = dist_np(Xs, Xs[7:8])[:, 0]
    nz = np.flatnonzero(quantise(mind))
    assert seeds_np(Xs, 7, np.array([0, 0], np.uint32), 2)[1] == nz[0]
    assert seeds_np(Xs, 7, np.array([0, 2 ** 32 - 1], np.uint32), 2)[1] == nz[-1]
    # total == 0: all votes identical -> index 0, every time, and one cluster
    same = np.repeat(Xs[:1], 30, axis=0)
    assert seeds_np(same, 11, r, 5).tolist() == [11, 0, 0, 0, 0]
    assert link_np(climb_np(same, same[[11, 0, 0]], 0.02, 3).astype(F32), 0.05).tolist() == [0, 0, 0]
    # fewer points than seeds; none
    assert len(seeds_np(Xs[:5], 9, r, 12)) == 5 and seeds_np(Xs[:5], 9, r, 12)[0] == 4 and len(seeds_np(Xs[:0], 0, r, 12)) == 0
    # a huge distance saturates q at 2^31 - 1
    assert quantise(np.array([0.0, 1e-7, 1.0, 3000.0], F32)).tolist() == [0, 0, 2 ** 20, 2 ** 31 - 1]


LITERAL_SEEDS = [7, 42, 61, 56, 55, 0, 16, 35, 18, 2, 26, 101]


def test_degenerate_frames():
    votes, fg, _ = vote_scene(24, 32, 3, seed=2)
    g = small_options(imp=IMP())
    r = np.arange(40, dtype=np.uint32) * 97654321
    empty = gms_np(votes, np.zeros_like(fg), 0, r, g)
    assert empty["report"].tolist() == [0] * 6 and not empty["ids"].any() and empty["centers"].shape == (0, 3) and len(empty["indices"]) == 0
    few = np.zeros_like(fg)
    few.reshape(-1)[np.flatnonzero(fg)[:23]] = 1             # n = 23, n_sub = 5 < num_seeds
    out = gms_np(votes, few, 3, r, small_options(min_pixels=5))
    assert out["info"].tolist() == [23, 5, 5] and len(out["indices"]) == 5 and out["report"][5] == 23 and out["report"][0] == out["report"][1] - out["report"][2] >= 1
    flat = votes.copy()
    flat[:] = flat[:, 5:6, 5:6]
    out = gms_np(flat, fg, 3, r, g)                          # total == 0: the seeds are 3, 0, 0, ...: one cluster
    assert out["indices"].tolist() == [3] + [0] * 39 and out["report"][1] == 1
    out = gms_np(votes, fg, 3, r, small_options(min_pixels=10 ** 4))
    assert out["report"][0] == 0 and out["report"][2] == out["report"][1] >= 3 and not out["ids"].any()
    # a far-away explicit seed keeps its position (every weight underflows to 0)
    _, Xs = compact_np(votes, fg, 5)
    far = np.array([[100.0, 100.0, 100.0]])
    np.testing.assert_array_equal(climb_np(Xs, far, 0.02, 10), far)


def test_chain_cases_reach_the_mode_branch():
    """The labels are asserted literally, and equal what the reference's own connected_components returned for the same seeds
    (tests/golden/gms_link_chains.npz, tools/gen_gms_golden.py)."""
    g = _golden("gms_link_chains.npz")
    for name, (Z, want) in chain_cases().items():
        Z64 = Z.astype(np.float64)
        dz = np.sqrt(((Z64[:, None] - Z64[None]) ** 2).sum(-1))
        assert np.abs(dz - 0.05).min() > 5e-3, name          # decidable: torch.norm and the pinned dist see the same balls
        assert link_np(Z, 0.05).tolist() == want, name
        np.testing.assert_array_equal(g[name + "_seeds"], Z)
        assert g[name + "_labels"].tolist() == want, name


FIXTURES = ["gms_scene_24x32.npz", "gms_scene_37x53.npz"]


def fixture_options(g):
    return GaussianMeanShift(num_seeds=int(g["num_seeds"]), sigma=float(g["sigma"]), iters=int(g["iters"]), epsilon=float(g["epsilon"]),
                             subsample=int(g["subsample"]), min_pixels=int(g["min_pixels"]), imp=None)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_with_the_contracts_seeds_equals_the_reference(name):
    """(a): the reference's own cluster() with select_smart_seeds returning the contract's seeds."""
    g = _golden(name)
    opt = fixture_options(g)
    out = gms_np(g["votes"], g["fg"], int(g["first"]), g["draws"], opt)
    np.testing.assert_array_equal(out["indices"], g["indices"])
    np.testing.assert_array_equal(out["seed_labels"], g["seed_labels"])
    np.testing.assert_array_equal(out["ids"], g["clustered"])
    # the reference climbs in float32: its own error against the float64 statement is the bar, and it is small
    ref_err = np.abs(g["seeds"].astype(np.float64) - climb_np(compact_np(g["votes"], g["fg"], opt.subsample)[1],
                                                              compact_np(g["votes"], g["fg"], opt.subsample)[1][g["indices"]], opt.sigma, opt.iters)).max()
    assert ref_err < 1e-5 and np.abs(out["seeds"].astype(np.float64) - g["seeds"]).max() <= ref_err + 2.0 ** -24 * np.abs(g["votes"]).max()
    bound = opt.num_seeds * 2.0 ** -24 * float(np.abs(g["votes"][:, g["fg"] != 0]).max())
    assert out["centers"].shape == g["centers"].shape and np.abs(out["centers"] - g["centers"]).max() <= bound
    assert out["report"][0] == g["clustered"].max() and out["report"][2] >= 1        # the strays were dropped by min_pixels


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_with_the_references_seeding_is_the_same_partition(name):
    """(b): the reference's own multinomial seeding."""
    g = _golden(name)
    opt = fixture_options(g)
    out = gms_np(g["votes"], g["fg"], int(g["first"]), g["draws"], opt)
    P, _ = compact_np(g["votes"], g["fg"], opt.subsample)
    assert decidable(P, out["seeds"], out["seed_labels"], opt.epsilon)
    assert same_partition(out["ids"], g["clustered_multinomial"])


def test_fixtures_are_small():
    names = [f for f in os.listdir(GOLDEN) if f.startswith("gms_")]
    assert len(names) >= 3 and all(os.path.getsize(os.path.join(GOLDEN, f)) < 600 * 1024 for f in names)


def test_ellipse_is_opencvs():
    from test_perturb_cpu import structuring_element
    assert ellipse(9).sum(1).tolist() == [1, 7, 7, 9, 9, 9, 7, 7, 1]
    for k in range(1, 16, 2):
        np.testing.assert_array_equal(ellipse(k), structuring_element(2, k))
        assert np.array_equal(ellipse(k), ellipse(k)[::-1, ::-1])            # symmetric: correlation and convolution agree


IMP_MAPS = [((48, 64), 5, 1), ((61, 83), 6, 2), ((96, 128), 7, 3)]


@pytest.mark.parametrize("shape,k,seed", IMP_MAPS)
def test_imp_against_scipy(shape, k, seed):
    ids = voronoi_map(*shape, k, seed)
    elem = ellipse(9).astype(bool)
    # the morphology, per mask, against scipy with OpenCV's border values
    m = ids == 1
    np.testing.assert_array_equal(morph_np(m, ellipse(9), True), ndimage.binary_erosion(m, elem, border_value=1))
    np.testing.assert_array_equal(morph_np(m, ellipse(9), False), ndimage.binary_dilation(m, elem, border_value=0))
    assert not morph_np(np.zeros(shape, bool), ellipse(9), True).any()       # an absent id is a no-op of the sequential loop
    # the whole IMP against the reference's loops restated with scipy
    want = ids.copy()
    for o in range(1, k + 1):
        mask = want == o
        opened = ndimage.binary_dilation(ndimage.binary_erosion(mask, elem, border_value=1), elem, border_value=0)
        res = ndimage.binary_erosion(ndimage.binary_dilation(opened, elem, border_value=0), elem, border_value=1)
        want[mask] = 0
        want[res] = o
    morphed = want.copy()
    comps_before = 0
    for o in range(1, k + 1):
        mask = want == o
        lab, n = ndimage.label(mask)                         # 4-connected; labels in raster order of the first pixel
        comps_before += n
        if n:
            sizes = ndimage.sum(mask, lab, range(1, n + 1))
            want[mask] = 0
            want[lab == 1 + int(np.argmax(sizes))] = o       # the first largest
    got, rep, keep = imp_np(ids, k, 9, True)
    assert keep == list(range(1, k + 1)) and rep.tolist() == [k, 0]
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(imp_np(ids, k, 9, False)[0], morphed)
    # the inputs exercise it: a tenth of the pixels and more change, eight and more components per id collapse to one
    comps_in = sum(ndimage.label(ids == o)[1] for o in range(1, k + 1))
    assert (got != ids).sum() > 0.1 * ids.size and comps_in >= 8 * k and comps_before >= k
    assert all(ndimage.label(got == o)[1] == 1 for o in range(1, k + 1))


def test_imp_drops_emptied_ids_and_renumbers():
    ids = np.zeros((40, 50), np.int32)
    ids[2:30, 2:30] = 1
    ids[10:13, 35:38] = 2                                    # smaller than the ellipse: the opening erases it
    ids[5:35, 40:49] = 4                                     # id 3 is absent
    ids[39, 0] = 9                                           # outside 0..n_ids: counts as 0
    got, rep, keep = imp_np(ids, 4, 9, True)
    assert keep == [1, 4] and rep.tolist() == [2, 1] and set(np.unique(got)) == {0, 1, 2}
    assert (got[9:31, 40:49] == 2).all() and (got[5:35, 44] == 2).all() and got[5, 40] == 0 and got[39, 0] == 0       # the opening rounds the corners
    got1, rep1, _ = imp_np(ids, 4, 1, False)                 # ksize 1: the identity
    assert rep1.tolist() == [3, 0] and np.array_equal(got1 > 0, (ids > 0) & (ids <= 4))


def test_header_declares_the_entries():
    txt = open(os.path.join(ROOT, "include", "quber_hip.h")).read()
    for name in ("seeds", "climb", "link", "assign", "imp", "cluster"):
        assert re.search(r"\bint quber_gms_%s\s*\(" % name, txt), name
    src = open(os.path.join(ROOT, "quber_amd", "csrc", "gms.hip")).read()
    assert "hipMemsetAsync" not in src and "cooperative" not in src.lower() and "hipMemcpy" not in src and "Synchronize" not in src
    assert "gms.hip" in open(os.path.join(ROOT, "quber_amd", "csrc", "Makefile")).read()
    from quber_amd import _lib
    for name in ("seeds", "climb", "link", "assign", "imp", "cluster"):
        assert "quber_gms_" + name in _lib.SIGNATURES
        decl = re.search(r"\bint quber_gms_%s\s*\(([^;]*)\);" % name, txt).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES["quber_gms_" + name][1]), name


def test_options():
    g = GaussianMeanShift()
    assert g.args() == (200, 0.02, 10, 0.05, 5, 300, IMP(9, True), 0) and GaussianMeanShift.uois() == g
    assert GaussianMeanShift.parse(None) is None and GaussianMeanShift.parse(g) is g and GaussianMeanShift(imp=None).imp is None
    assert GaussianMeanShift(seed=3) == GaussianMeanShift(seed=3) != GaussianMeanShift(seed=4) and "num_seeds=200" in repr(g)
    assert IMP().args() == (9, True) and IMP(3, False) != IMP(3, True) and "ksize=9" in repr(IMP()) and g.n_sub(11) == 3
    # the stream: per frame the first seed, then num_seeds - 1 32-bit draws, in frame order
    rs = np.random.RandomState(7)
    want = []
    for ns in (100, 0, 7):
        f = rs.randint(0, max(ns, 1))
        want.append((f, rs.randint(0, 2 ** 32, size=3, dtype=np.uint64).astype(np.uint32).tolist()))
    g7 = GaussianMeanShift(num_seeds=4, seed=7)
    f1, r1 = g7.draws([100])
    f2, r2 = g7.draws([0, 7])
    assert [(int(f), r[1:].tolist()) for f, r in zip(list(f1) + list(f2), list(r1) + list(r2))] == want and r1.dtype == np.uint32
    g7.reseed()
    assert g7.draws([100])[0][0] == want[0][0]
    for bad in (dict(num_seeds=0), dict(num_seeds=MAX_SEEDS + 1), dict(num_seeds=2.5), dict(sigma=0), dict(sigma="x"), dict(iters=-1),
                dict(epsilon=-0.1), dict(subsample=0), dict(min_pixels=-1), dict(seed=-1), dict(sigma=float("nan")), dict(imp=9)):
        with pytest.raises(ValueError):
            GaussianMeanShift(**bad)
    for bad in (dict(ksize=8), dict(ksize=17), dict(ksize=0), dict(ksize=2.5), dict(largest=1)):
        with pytest.raises(ValueError):
            IMP(**bad)
    with pytest.raises(ValueError):
        GaussianMeanShift.parse("uois")
    assert imp_plane_bytes(480, 640) == 76800 and imp_plane_bytes(61, 83) == 2 * 61 * 3 * 4


def test_refine_options_take_either_clusterer():
    from quber_amd.maskrefiner.predictor import RefineOptions
    from quber_amd.masknms import MaskNMS
    from quber_amd.meanshift import MeanShift
    from quber_amd.zoom import ZoomIn
    g, ms = GaussianMeanShift(), MeanShift()
    assert RefineOptions.parse(cluster=g).cluster is g and RefineOptions.parse(cluster=ms).cluster is ms and RefineOptions.parse().cluster is None
    with pytest.raises(ValueError):
        RefineOptions.parse(cluster=g, nms=MaskNMS())
    with pytest.raises(ValueError):
        RefineOptions.parse(cluster="gms")
    zoomed = RefineOptions.parse(cluster=g, zoom=ZoomIn(), tta=True)
    assert zoomed.cluster is g and zoomed.for_crops().cluster is None and zoomed.for_crops().tta      # the crop pass is given masks
