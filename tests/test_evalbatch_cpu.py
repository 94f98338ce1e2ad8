"""CPU: the host half of the batched evaluation (quber_amd/eval/evaluation.py: enqueue_metrics / collect_metrics, csrc/evalbatch.hip).

`score_matrix_np` and `gather_np` state in numpy what stages 3-5 of quber_eval_batch deliver (tests/test_gpu_evalbatch.py holds the
device to them); the shared final arithmetic `_metrics_from_tables` is fed tables made here with numpy and the oracle's solver and
must reproduce the reference's dictionaries exactly.  Every comparison is `==`."""
import json

import numpy as np
import pytest

from conftest import golden
from oracle import metrics_np
from oracle.assign_py import assign as oracle_assign
from quber_amd import synth


def tables_np(pred, gt):
    """-> (labels_pred, labels_gt, table[n_gt, n_pred]) with np.unique ordering: what stage 1 delivers."""
    lp, lg = np.unique(pred), np.unique(gt)
    table = np.zeros((len(lg), len(lp)), np.int64)
    np.add.at(table, (np.searchsorted(lg, np.asarray(gt).ravel()), np.searchsorted(lp, np.asarray(pred).ravel())), 1)
    return lp.astype(np.int64), lg.astype(np.int64), table


def score_matrix_np(lp, lg, table):
    """Stage 3: multilabel_metrics lines 102-110 over the non-background labels in float64 -> (F [gt objects, predicted objects],
    cost = F.max() - F), or (None, None) when a side has no object."""
    kp, kg = lp != 0, lg != 0
    if not kp.any() or not kg.any():
        return None, None
    tps = table[np.ix_(kg, kp)].astype(np.float64)
    ap, ag = table.sum(axis=0)[kp].astype(np.float64), table.sum(axis=1)[kg].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        P, R = tps / ap[None, :], tps / ag[:, None]
        F = (2 * P * R) / (P + R)
    F[np.isnan(F)] = 0
    return F, F.max() - F


def gather_np(lp, lg, table, assignment, ptps=None, rtps=None):
    """Stage 5: per assigned pair (gt object, predicted object), in row order: overlap, union and the boundary true positives."""
    kp, kg = lp != 0, lg != 0
    tps = table[np.ix_(kg, kp)]
    ap, ag = table.sum(axis=0)[kp], table.sum(axis=1)[kg]
    out = {"pairs": [(int(i), int(j)) for i, j in assignment],
           "pair_tps": np.array([tps[i, j] for i, j in assignment], np.int64),
           "pair_union": np.array([ag[i] + ap[j] - tps[i, j] for i, j in assignment], np.int64)}
    if ptps is not None:
        out["pair_ptps"] = np.array([ptps[i, j] for i, j in assignment], np.int64)
        out["pair_rtps"] = np.array([rtps[i, j] for i, j in assignment], np.int64)
    return out


def boundary_np(pred, gt, lp, lg):
    """-> (bc_pred, bc_gt, ptps, rtps) as float64, like boundary_counts, from the oracle's per-pair functions."""
    op, og = lp[lp != 0], lg[lg != 0]
    bc_p = np.array([metrics_np.seg2bmap(pred == v).sum() for v in op], np.float64)
    bc_g = np.array([metrics_np.seg2bmap(gt == v).sum() for v in og], np.float64)
    ptps, rtps = np.zeros((len(og), len(op))), np.zeros((len(og), len(op)))
    for i, gv in enumerate(og):
        for j, pv in enumerate(op):
            ptps[i, j], rtps[i, j] = metrics_np.boundary_overlap(pred == pv, gt == gv)
    return bc_p, bc_g, ptps, rtps


def metrics_via_tables(pred, gt, with_boundary):
    from quber_amd.eval.evaluation import _metrics_from_tables
    lp, lg, table = tables_np(pred, gt)
    F, cost = score_matrix_np(lp, lg, table)
    assignment = oracle_assign(cost) if F is not None else []
    boundary = boundary_np(pred, gt, lp, lg) if with_boundary and F is not None else None
    if with_boundary and F is None:
        boundary = lambda *_: pytest.fail("boundary work asked for a frame without objects on both sides")
    return _metrics_from_tables(lp, lg, table, assignment, boundary)


def same_dicts(got, exp):
    assert set(got) == set(exp)
    for k, v in exp.items():
        if v is None:
            assert got[k] is None, k
        else:
            assert float(got[k]) == float(v), (k, got[k], v)


@pytest.mark.parametrize("path", golden("metrics"), ids=lambda p: p.split("metrics_")[-1])
def test_final_arithmetic_reproduces_reference_results(path):
    z = np.load(path)
    same_dicts(metrics_via_tables(z["pred"], z["gt"], False), json.loads(str(z["result"])))


def test_all_eight_reference_fixtures_are_there():
    assert len(golden("metrics")) == 8


@pytest.mark.parametrize("h,w,n,seed", [(75, 101, 4, 2), (96, 128, 5, 1)])
def test_final_arithmetic_reproduces_oracle_with_boundary(h, w, n, seed):
    gtm, initm = synth.make_masks(np.random.default_rng(seed), n, h, w)
    gt, pred = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for i in range(n):
        gt[gtm[i]] = i + 2
        pred[initm[i]] = i + 1
    same_dicts(metrics_via_tables(pred, gt, True), metrics_np.multilabel_metrics(pred, gt, compute_boundary_stuff=True))


def test_solver_is_called_only_without_an_assignment(monkeypatch):
    """With an assignment given (the batched path) the host solver does not run; without one (the per-frame path) it does."""
    from quber_amd.eval import evaluation
    z = np.load([p for p in golden("metrics") if "scene_a" in p][0])
    lp, lg, table = tables_np(z["pred"], z["gt"])
    _, cost = score_matrix_np(lp, lg, table)
    want = evaluation._metrics_from_tables(lp, lg, table, None, None)
    calls = []
    monkeypatch.setattr(evaluation, "munkres_assign", lambda c: calls.append(1) or oracle_assign(c))
    same_dicts(evaluation._metrics_from_tables(lp, lg, table, oracle_assign(cost), None), want)
    assert not calls
    same_dicts(evaluation._metrics_from_tables(lp, lg, table, None, None), want)
    assert calls == [1]


def test_gather_contract_matches_the_sums_the_dict_uses():
    z = np.load([p for p in golden("metrics") if "scene_c" in p][0])
    lp, lg, table = tables_np(z["pred"], z["gt"])
    F, cost = score_matrix_np(lp, lg, table)
    g = gather_np(lp, lg, table, oracle_assign(cost))
    exp = json.loads(str(z["result"]))
    assert len(g["pairs"]) == min(F.shape)
    assert np.sum(g["pair_tps"].astype(np.float64)) / np.sum(g["pair_union"].astype(np.float64)) == exp["obj_mIOU"]


def test_record_layout_is_aligned_and_disjoint():
    from quber_amd.eval.evaluation import record_layout
    for cap in (1, 3, 16, 64, 255, 256):
        off, size = record_layout(cap)
        order = sorted(off.values())
        assert order == list(off.values()) and size % 8 == 0 and size >= order[-1] + 4 * cap
        assert all(off[k] % 8 == 0 for k in ("table", "F", "area", "pair_tps", "pair_union")) and all(v % 4 == 0 for v in order)
        assert size == (24 * cap * cap + 68 * cap + 32 + 7) // 8 * 8          # the formula include/quber_hip.h states


def test_label_map_from_masks_is_the_reference_paint_loop():
    from quber_amd.eval.refiner_model import label_map_from_masks
    rng = np.random.default_rng(0)
    masks = np.zeros((5, 40, 56), bool)
    for i in range(5):                                   # overlapping rectangles: later masks must end on top
        y, x = int(rng.integers(0, 20)), int(rng.integers(0, 30))
        masks[i, y:y + 18, x:x + 24] = True
    anno = np.zeros((40, 56), np.uint8)
    for form in (masks, masks.astype(np.uint8) * 255, list(masks)):
        exp = np.zeros_like(anno)
        for i, mask in enumerate(form):
            exp[mask > False] = i + 1
        got = label_map_from_masks(form, anno.shape)
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got, exp)
    assert (masks.sum(0) > 1).any() and len(np.unique(exp)) == 6
    for empty in ([], np.zeros((0, 40, 56), bool)):      # no masks at all (the adapter returns [] then)
        np.testing.assert_array_equal(label_map_from_masks(empty, anno.shape), np.zeros((40, 56), np.int32))


def test_load_annotation_zeroes_the_ocid_background_labels():
    from quber_amd.eval.refiner_model import H, W, load_annotation
    anno = (np.arange(H * W).reshape(H, W) % 6).astype(np.uint8)
    keep = anno.copy()
    table = load_annotation(anno, "OCID-dataset/ARID20/table/top/seq08/rgb/a.png", "OCID")
    floor = load_annotation(anno, "OCID-dataset/ARID20/floor/top/seq08/rgb/a.png", "OCID")
    np.testing.assert_array_equal(table, np.where(keep <= 2, 0, keep))
    np.testing.assert_array_equal(floor, np.where(keep <= 1, 0, keep))
    np.testing.assert_array_equal(load_annotation(anno, "OSD/image_color/learn0.png", "OSD"), keep)
    np.testing.assert_array_equal(anno, keep)            # the caller's array is left alone
    with pytest.raises(ValueError):
        load_annotation(anno, "OCID-dataset/somewhere/else.png", "OCID")
    with pytest.raises(ValueError):                      # another size needs the resize function
        load_annotation(anno[:100], "x/table/a.png", "OCID")
    # a 16-bit annotation of another size goes through an 8-bit nearest resize as two byte planes
    small = (np.arange(240 * 320).reshape(240, 320) * 7 % 1000).astype(np.uint16)
    nearest = lambda img, h, w, linear: img[(np.arange(h) * img.shape[0] // h)[:, None], (np.arange(w) * img.shape[1] // w)[None, :]]
    got = load_annotation(small, "q.png", "OSD", nearest)
    assert got.dtype == np.uint16
    np.testing.assert_array_equal(got, nearest(small, H, W, False))
