"""CPU: the contract of the mean-shift clustering of a UCN embedding map into initial masks (csrc/meanshift.hip, Engine.meanshift,
MaskRefinerPredictor(cluster=MeanShift())), stated in numpy, and what can be checked of the feature without a GPU.

The reference (eval/base_model.py:622-840, cosine metric): ``select_smart_seeds`` picks num_seeds pixels farthest-first from a random
first one, ``seed_hill_climbing_ball`` moves them max_iters times to the normalised mean of all pixels weighted by exp(kappa cos),
``connected_components`` gives seeds within epsilon = 2 alpha of one another the same label, every pixel takes the label of its
nearest seed, the largest cluster becomes label 0; ``filter_labels_depth`` (:34-47) drops the labels with too few pixels of positive
depth, and ``predict`` numbers what is left 1..count.  ``meanshift_np`` / ``filter_depth_np`` restate this in the arithmetic the
device reproduces; tests/golden/meanshift_*.npz (tools/gen_meanshift_golden.py) were recorded from the reference's own functions.

Where the contract pins what the reference leaves open:
  * every dot product that DECIDES something (seed choice, seed linking, pixel assignment) is accumulated in float32 in channel order
    0..63, multiply and add rounded separately; the reference's torch.mm leaves the order to the BLAS build.  On the grid fixtures
    every such product and sum is exact, so the two agree bit for bit; on the blob fixtures near-ties may choose other seeds and the
    comparison is of partitions.
  * the first seed of a frame is an argument (the reference draws it from numpy's global stream).
  * the climb is stated in float64 on the float32 inputs; the device computes it in float32 and is held to 4 x the error of torch's own
    float32 mm / exp against this statement (tests/test_gpu_meanshift.py).
  * a seed label of -1 (a seed outside its own epsilon ball: a zero vector) stays -1, and a pixel that takes it belongs to no mask.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from quber_amd.meanshift import CHANNELS, MAX_SEEDS, MeanShift

GOLDEN = os.path.join(ROOT, "tests", "golden")
F32 = np.float32


# ---- the contract ----
def pinned_dot(A, Bm):
    """A f32 [m,d], Bm f32 [k,d] -> f32 [m,k]: sum over c = 0..d-1 in that order, multiply and add rounded separately."""
    A, Bm = np.asarray(A, F32), np.asarray(Bm, F32)
    acc = np.zeros((A.shape[0], Bm.shape[0]), F32)
    for c in range(A.shape[1]):
        acc = acc + A[:, c:c + 1] * Bm[None, :, c]
    return acc


def cos_dist(A, Bm):
    return F32(0.5) * (F32(1) - pinned_dot(A, Bm))


def seeds_np(X, first, num_seeds):
    """X f32 [n,d] -> i32 [num_seeds]: farthest-first, the first index of the maximum of the running minimum distance."""
    idx = np.empty(num_seeds, np.int32)
    idx[0] = first
    mind = cos_dist(X, X[first:first + 1])[:, 0]
    for k in range(1, num_seeds):
        idx[k] = int(np.argmax(mind))
        mind = np.minimum(mind, cos_dist(X, X[idx[k]:idx[k] + 1])[:, 0])
    return idx


def climb_np(X, Z, kappa, iters):
    """float64: iters times Z = normalize(exp(kappa Z X^T) X) (F.normalize: x / max(|x|, 1e-12))."""
    X64, Z = np.asarray(X, np.float64), np.asarray(Z, np.float64)
    for _ in range(iters):
        Z = np.exp(kappa * (Z @ X64.T)) @ X64
        Z = Z / np.maximum(np.linalg.norm(Z, axis=1, keepdims=True), 1e-12)
    return Z


def link_np(Z, epsilon):
    """Z f32 [S,d] -> i32 [S]: connected_components (base_model.py:737-770) as written, quirks included."""
    Z = np.asarray(Z, F32)
    near = cos_dist(Z, Z) <= F32(epsilon)
    S = Z.shape[0]
    labels = -np.ones(S, np.int32)
    K = 0
    for i in range(S):
        if labels[i] != -1:
            continue
        comp = near[:, i]
        seen = labels[comp]
        if len(np.unique(seen)) > 1:                         # "more than one distinct label, -1 included"
            vals, counts = np.unique(seen[seen != -1], return_counts=True)
            label = vals[np.argmax(counts)]                  # get_label_mode: the smallest label among equal counts
        else:
            label = K
            K += 1
        labels[comp] = label
    return labels


def assign_np(X, Z, seed_labels):
    """-> (nearest i32 [n]: first index of the minimum distance, labels i32 [n] after the largest of the labels 0..num-1 swapped with 0)."""
    nearest = np.argmin(cos_dist(X, np.asarray(Z, F32)), axis=1).astype(np.int32)
    lab = np.asarray(seed_labels, np.int32)[nearest]
    num = len(np.unique(seed_labels))                        # (a vanished label or a -1 makes this differ from max + 1: the reference's quirk)
    count = np.array([(lab == i).sum() for i in range(num)])
    big = int(np.argmax(count))
    if big != 0:
        i0, i1 = lab == 0, lab == big
        lab[i0], lab[i1] = big, 0
    return nearest, lab


def filter_depth_np(labels, z=None, threshold=None, max_masks=None):
    """labels i32 [n] (assign_np), z f32 [n] or None -> (ids i32 [n]: 0, 1..count; report i32 [4]: count, clusters before the filter,
    dropped by depth, truncated).  A label < 0 is no cluster.  Survivors are renumbered in ascending label order; those behind
    max_masks are dropped and reported as truncated."""
    labels = np.asarray(labels, np.int32)
    ids = np.zeros_like(labels)
    found = [int(l) for l in np.unique(labels) if l > 0]
    keep = []
    for l in found:
        m = labels == l
        if z is not None and threshold is not None:
            if F32((np.asarray(z, F32)[m] > 0).sum()) / F32(m.sum()) < F32(threshold):
                continue
        keep.append(l)
    dropped = len(found) - len(keep)
    truncated = int(max_masks is not None and len(keep) > max_masks)
    if truncated:
        keep = keep[:max_masks]
    for k, l in enumerate(keep):
        ids[labels == l] = k + 1
    return ids, np.array([len(keep), len(found), dropped, truncated], np.int32)


def meanshift_np(X, first, num_seeds=100, kappa=20.0, iters=10, epsilon=0.04):
    """One frame.  X f32 [n,64] -> dict: indices i32 [S], seeds f32 [S,64] (the climbed modes, float64 rounded once), seed_labels i32
    [S], nearest i32 [n], labels i32 [n] (the reference's cluster_labels)."""
    X = np.ascontiguousarray(X, F32)
    idx = seeds_np(X, first, num_seeds)
    Z = climb_np(X, X[idx], kappa, iters).astype(F32)
    sl = link_np(Z, epsilon)
    nearest, lab = assign_np(X, Z, sl)
    return {"indices": idx, "seeds": Z, "seed_labels": sl, "nearest": nearest, "labels": lab}


def cluster_np(emb, first, ms, depth_z=None, max_masks=None):
    """The chain on one frame: emb f32 [64,H,W] -> dict with ids i32 [H,W], masks u8 [max_masks,H,W] of 0 / 255, report, + meanshift_np's."""
    c, h, w = emb.shape
    r = meanshift_np(emb.reshape(c, h * w).T, first, ms.num_seeds, ms.kappa, ms.iters, ms.epsilon)
    z = None if depth_z is None else np.asarray(depth_z, F32).reshape(-1)
    ids, rep = filter_depth_np(r["labels"], z, ms.depth_threshold, max_masks)
    n_out = int(rep[0]) if max_masks is None else max_masks
    masks = np.stack([(ids == k + 1) for k in range(n_out)]).reshape(n_out, h, w).astype(np.uint8) * 255 if n_out else np.zeros((0, h, w), np.uint8)
    return dict(r, ids=ids.reshape(h, w), masks=masks, report=rep)


def decidable(X, Z, seed_labels, epsilon, margin=1e-3):
    """What the chain tests require of an input before they ask for equal label maps: every seed-to-seed distance is more than `margin`
    away from epsilon, and for every pixel the nearest seed of any other cluster is more than `margin` farther than that of its own."""
    Z64, X64 = np.asarray(Z, np.float64), np.asarray(X, np.float64)
    dz = 0.5 * (1 - Z64 @ Z64.T)
    if np.abs(dz - epsilon).min() <= margin:
        return False
    d = 0.5 * (1 - X64 @ Z64.T)
    labs = np.unique(seed_labels)
    per = np.stack([d[:, seed_labels == l].min(axis=1) for l in labs], axis=1)
    per.sort(axis=1)
    return per.shape[1] == 1 or bool((per[:, 1] - per[:, 0]).min() > margin)


def same_partition(a, b):
    """Two label maps describe the same partition with label 0 on the same cluster."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    pairs = {(int(x), int(y)) for x, y in zip(a, b)}
    return len({x for x, _ in pairs}) == len(pairs) == len({y for _, y in pairs}) and np.array_equal(a == 0, b == 0)


# ---- inputs ----
def blob_embeddings(h, w, k, seed, noise=0.05):
    """f32 [64,h,w], float16-representable: unit vectors around k well-separated directions, in vertical stripes of unequal width (the
    first is the widest: the background)."""
    rng = np.random.RandomState(seed)
    dirs = np.linalg.qr(rng.randn(CHANNELS, CHANNELS))[0][:k]
    edges = np.linspace(0, w, 2 * k + 1)[[0] + list(range(k + 1, 2 * k + 1))] if k > 1 else np.array([0, w])
    col = np.clip(np.searchsorted(edges, np.arange(w), side="right") - 1, 0, k - 1)
    which = np.broadcast_to(col[None, :], (h, w)).reshape(-1)
    x = dirs[which] + noise * rng.randn(h * w, CHANNELS) / np.sqrt(CHANNELS)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x.astype(np.float16).astype(F32).T.reshape(CHANNELS, h, w)), which.reshape(h, w)


def grid_embeddings(h, w, k, seed):
    """f32 [64,h,w]: rows with four non-zero entries that are multiples of 2^-6, norm <= 1 - every float32 dot product of two rows is
    exact in any summation order.  Cluster j owns channels 8 j .. 8 j + 7: three large entries and one small one that varies."""
    rng = np.random.RandomState(seed)
    which = rng.randint(0, k, h * w)
    which[rng.rand(h * w) < 0.4] = 0
    x = np.zeros((h * w, CHANNELS), F32)
    rows = np.arange(h * w)
    for j in range(3):
        x[rows, 8 * which + j] = (32 + rng.randint(-2, 3, h * w)) / 64.0
    x[rows, 8 * which + 3 + rng.randint(0, 5, h * w)] = rng.randint(1, 9, h * w) / 64.0
    assert (np.linalg.norm(x, axis=1) <= 1).all()
    return np.ascontiguousarray(x.T.reshape(CHANNELS, h, w)), which.reshape(h, w)


def hand_cases():
    """name -> (Z f32 [S,64] climbed seeds, X f32 [n,64], z f32 [n] or None, threshold): link / assign / filter inputs built by hand."""
    e = np.eye(CHANNELS, dtype=F32)
    rng = np.random.RandomState(5)
    px = lambda rows, reps: np.repeat(np.asarray(rows, F32), reps, axis=0)
    out = {}
    # a seed that is a zero vector lies outside its own ball: it takes a label number with it (1 vanishes) and stays -1
    Z = np.stack([e[0], np.zeros(CHANNELS, F32), e[1], e[1], e[0]])
    out["vanishing_label"] = (Z, px([e[0], e[1]], [5, 9]), None, None)
    out["one_cluster"] = (np.stack([e[3]] * 4), px([e[3]], [12]), None, None)
    same = (rng.randint(-8, 9, CHANNELS) / 64.0).astype(F32)
    out["all_identical"] = (np.stack([same] * 3), px([same], [17]), None, None)
    Z = np.stack([e[0], e[1], e[2], e[1]])
    X = px([e[0], e[1], e[2]], [20, 10, 5])
    z = np.ones(35, F32)
    z[20:28] = 0            # label of e[1]: 2 of 10 pixels with depth -> dropped at 0.5; e[2]: all 5 -> kept
    z[0:20] = -1            # the background's depth does not matter
    out["depth_drops_one"] = (Z, X, z, 0.5)
    for name, (Z, _) in chain_cases().items():               # one pixel group per seed direction, 14 pixels in all
        out[name] = (Z, px(Z / np.linalg.norm(Z, axis=1, keepdims=True), [3, 2, 4, 1, 2, 2]), None, None)
    return out


def chain_cases():
    """name -> (Z f32 [6,64], the seed labels connected_components gives them): seed sets whose epsilon balls are NOT transitive, so that
    the labelling meets seeds that already carry labels - the mode branch, which collapsed seeds never reach.  Seeds lie in the plane of
    channels 0 and 1 at the given angles; epsilon = 0.04 is an angle of 23.07 degrees between unit vectors, and no distance below is
    within 3e-3 of it.  Named k, o, j, m1, m2, i: k's ball holds j but not i; o's ball holds m1 (and m2); i, the last seed, is in nobody's
    ball and its own holds j and m1 (and m2).
    With distances that are symmetric and seeds inside their own balls (every set but the last) the seed that opens a label keeps it: only
    an unlabelled seed re-labels, and whatever holds the opener in its ball was labelled by the opener.  A label vanishes by re-labelling
    only when its opener lies outside its own ball - the last set, where k is short (norm 0.9) and j long (1.25)."""
    def seeds(*polar):
        Z = np.zeros((len(polar), CHANNELS), np.float64)
        for r, (deg, norm) in enumerate(polar):
            Z[r, 0], Z[r, 1] = norm * np.cos(np.deg2rad(deg)), norm * np.sin(np.deg2rad(deg))
        return Z.astype(F32)
    u = lambda deg: (deg, 1.0)
    return {
        # i meets j (label 0) and m1, m2 (label 1): the mode, 1, wins over the smaller label and j is re-labelled
        "chain_mode": (seeds(u(0), u(80), u(20), u(60), u(62), u(40)), [0, 1, 1, 1, 1, 1]),
        # m2 out of i's reach: one seed of each label, equal counts -> the smallest label, 0; m1 is re-labelled
        "chain_tie": (seeds(u(0), u(80), u(20), u(60), u(70), u(40)), [0, 1, 0, 0, 1, 0]),
        # the same tie with o before k, so that the seed i meets FIRST (j, index 2) carries the larger label: still the smallest label
        "chain_tie_order": (seeds(u(80), u(0), u(20), u(60), u(70), u(40)), [0, 1, 0, 0, 0, 0]),
        # k outside its own ball opens label 0 for j alone and stays -1; i re-labels j: label 0 has vanished
        "chain_vanish": (seeds((0, 0.9), u(80), (20, 1.25), u(60), u(62), u(40)), [-1, 1, 1, 1, 1, 1]),
    }


# ---- tests ----
def test_contract_properties_on_blobs():
    emb, which = blob_embeddings(24, 32, 4, seed=1)
    X = emb.reshape(CHANNELS, -1).T
    r = meanshift_np(X, 17, num_seeds=33)
    assert r["indices"][0] == 17 and len(set(r["indices"].tolist())) == 33
    assert len(np.unique(r["seed_labels"])) == 4 and same_partition(r["labels"], which.ravel())
    assert decidable(X, r["seeds"], r["seed_labels"], 0.04)
    ids, rep = filter_depth_np(r["labels"])
    assert rep.tolist() == [3, 3, 0, 0] and sorted(np.bincount(ids)[1:].tolist()) == sorted(np.bincount(which.ravel())[1:].tolist())
    z = (which.ravel() != 2).astype(F32)
    ids2, rep2 = filter_depth_np(r["labels"], z, 0.5)
    assert rep2.tolist() == [2, 3, 1, 0] and not ids2[which.ravel() == 2].any()
    assert filter_depth_np(r["labels"], max_masks=2)[1].tolist() == [2, 3, 0, 1]


def test_hand_cases():
    c = hand_cases()
    Z, X, _, _ = c["vanishing_label"]
    sl = link_np(Z, 0.04)
    assert sl.tolist() == [0, -1, 2, 2, 0]                   # label 1 went with the zero seed
    _, lab = assign_np(X, Z, sl)
    assert lab[:5].tolist() == [2] * 5 and lab[5:].tolist() == [0] * 9       # num = 3 counts labels 0..2: the 9 pixels of label 2 win
    Z, X, _, _ = c["one_cluster"]
    assert link_np(Z, 0.04).tolist() == [0] * 4
    assert filter_depth_np(assign_np(X, Z, link_np(Z, 0.04))[1])[1].tolist() == [0, 0, 0, 0]
    Z, X, _, _ = c["all_identical"]
    assert filter_depth_np(assign_np(X, Z, link_np(Z, 0.04))[1])[0].max() == 0
    Z, X, z, thr = c["depth_drops_one"]
    sl = link_np(Z, 0.04)
    assert sl.tolist() == [0, 1, 2, 1]
    ids, rep = filter_depth_np(assign_np(X, Z, sl)[1], z, thr)
    assert rep.tolist() == [1, 2, 1, 0] and ids[30:].tolist() == [1] * 5 and not ids[:30].any()


def test_chain_cases_reach_the_mode_branch():
    """The labels are asserted literally, and equal what the reference's own connected_components returned for the same seeds
    (tests/golden/meanshift_link_chains.npz, tools/gen_meanshift_golden.py)."""
    g = _golden("meanshift_link_chains.npz")
    for name, (Z, want) in chain_cases().items():
        dz = 0.5 * (1 - Z.astype(np.float64) @ Z.astype(np.float64).T)
        assert np.abs(dz - 0.04).min() > 3e-3, name          # decidable: torch.mm and the pinned dot see the same balls
        assert link_np(Z, 0.04).tolist() == want, name
        np.testing.assert_array_equal(g[name + "_seeds"], Z)
        assert g[name + "_labels"].tolist() == want, name
    # what the pixels make of it: in chain_vanish num = 2 ({-1, 1}) counts labels 0 and 1 only
    Z, X, _, _ = hand_cases()["chain_vanish"]
    nearest, lab = assign_np(X, Z, link_np(Z, 0.04))
    assert set(lab.tolist()) <= {-1, 0} and (lab == 0).sum() == (nearest != 0).sum()       # label 1, the largest, became 0
    Z, X, _, _ = hand_cases()["chain_tie"]
    assert filter_depth_np(assign_np(X, Z, link_np(Z, 0.04))[1])[1].tolist() == [1, 1, 0, 0]


def _golden(name):
    return np.load(os.path.join(GOLDEN, name))


@pytest.mark.parametrize("name", ["meanshift_grid_24x32.npz", "meanshift_grid_37x53.npz"])
def test_grid_fixture_equals_reference_exactly(name):
    g = _golden(name)
    emb = g["emb"].astype(F32)
    X = emb.reshape(CHANNELS, -1).T
    r = meanshift_np(X, int(g["indices"][0]), int(g["num_seeds"]), float(g["kappa"]), int(g["iters"]), float(g["epsilon"]))
    np.testing.assert_array_equal(r["indices"], g["indices"])
    np.testing.assert_array_equal(r["seed_labels"], g["seed_labels"])
    np.testing.assert_array_equal(r["labels"].reshape(emb.shape[1:]), g["labels"])
    assert np.abs(r["seeds"] - g["seeds"]).max() < 1e-5       # (the reference climbs in float32)
    ids, rep = filter_depth_np(r["labels"], g["depth_z"].reshape(-1), float(g["threshold"]))
    np.testing.assert_array_equal(ids.reshape(emb.shape[1:]), g["filtered"])
    assert rep[0] == len(np.unique(g["filtered"])) - 1 and rep[2] >= 1


@pytest.mark.parametrize("name", ["meanshift_blob_24x32.npz", "meanshift_blob_37x53.npz"])
def test_blob_fixture_equals_reference_as_partition(name):
    g = _golden(name)
    emb = g["emb"].astype(F32)
    X = emb.reshape(CHANNELS, -1).T
    r = meanshift_np(X, int(g["indices"][0]), int(g["num_seeds"]), float(g["kappa"]), int(g["iters"]), float(g["epsilon"]))
    assert decidable(X, r["seeds"], r["seed_labels"], float(g["epsilon"]))
    assert same_partition(r["labels"], g["labels"])
    # the climbed modes per cluster: every seed of a cluster has collapsed onto one mode, the reference's and the contract's alike
    for l in np.unique(g["labels"]):
        px = np.flatnonzero(g["labels"].ravel() == l)[0]
        mine = r["seeds"][r["nearest"][px]]
        theirs = g["seeds"][np.argmin(0.5 * (1 - g["seeds"].astype(np.float64) @ X[px].astype(np.float64)))]
        assert np.abs(mine - theirs).max() < 1e-5
    ids, _ = filter_depth_np(r["labels"], g["depth_z"].reshape(-1), float(g["threshold"]))
    assert same_partition(ids, g["filtered"])


def test_fixtures_are_small():
    names = [f for f in os.listdir(GOLDEN) if f.startswith("meanshift_")]
    assert len(names) >= 4 and all(os.path.getsize(os.path.join(GOLDEN, f)) < 600 * 1024 for f in names)


def test_header_declares_the_entries():
    txt = open(os.path.join(ROOT, "include", "quber_hip.h")).read()
    for name in ("seeds", "climb", "link", "assign", "cluster"):
        assert re.search(r"\bint quber_meanshift_%s\s*\(" % name, txt), name
    src = open(os.path.join(ROOT, "quber_amd", "csrc", "meanshift.hip")).read()
    assert "mfma_f32_32x32x2f32" in src and "hipMemsetAsync" not in src and "cooperative" not in src.lower()
    assert "meanshift.hip" in open(os.path.join(ROOT, "quber_amd", "csrc", "Makefile")).read()


def test_options():
    ms = MeanShift()
    assert ms.args() == (100, 20.0, 10, 0.02, None, 0) and ms.epsilon == 0.04 and MeanShift.parse(None) is None and MeanShift.parse(ms) is ms
    assert MeanShift.ucn("OSD").depth_threshold == 0.8 and MeanShift.ucn("OCID").depth_threshold == 0.5
    assert MeanShift.ucn("HOPE").depth_threshold == 0.5 and MeanShift.ucn("DoPose").depth_threshold == 0.5 and MeanShift.ucn("TOD").depth_threshold is None
    assert MeanShift(seed=3) == MeanShift(seed=3) and MeanShift(seed=3) != MeanShift(seed=4) and "num_seeds=100" in repr(ms)
    rs = np.random.RandomState(7)
    want = [rs.randint(0, 768) for _ in range(5)]
    m7 = MeanShift(seed=7)
    assert m7.first_seeds(2, 768).tolist() + m7.first_seeds(3, 768).tolist() == want       # one draw per frame, in frame order
    for bad in (dict(num_seeds=0), dict(num_seeds=MAX_SEEDS + 1), dict(num_seeds=2.5), dict(kappa="x"), dict(iters=-1), dict(alpha=-0.1),
                dict(depth_threshold=1.5), dict(seed=-1), dict(kappa=float("nan"))):
        with pytest.raises(ValueError):
            MeanShift(**bad)
    with pytest.raises(ValueError):
        MeanShift.parse("ucn")
    from quber_amd.maskrefiner.predictor import RefineOptions
    o = RefineOptions.parse(cluster=ms)
    assert o.cluster is ms and RefineOptions.parse().cluster is None
    from quber_amd.masknms import MaskNMS
    with pytest.raises(ValueError):
        RefineOptions.parse(cluster=ms, nms=MaskNMS())
    from quber_amd.zoom import ZoomIn
    zoomed = RefineOptions.parse(cluster=ms, zoom=ZoomIn(), tta=True)
    assert zoomed.cluster is ms and zoomed.for_crops().cluster is None and zoomed.for_crops().tta      # the crop pass is given masks
    with pytest.raises(ValueError):
        MeanShift(kappa=64.5)                                # exp(kappa) summed over 2^24 pixels must stay inside float32
