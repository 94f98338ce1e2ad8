"""GPU: the batched evaluation (csrc/evalbatch.hip, quber_amd/eval/evaluation.py:enqueue_metrics / collect_metrics) - the solver alone
against the golden cases and the oracle's solver, every stage of the whole call against its numpy statement, every dictionary against
the per-frame function and the oracle.  Every comparison is exact."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden
from oracle import metrics_np
from oracle.assign_py import assign as oracle_assign
from quber_amd import _lib, synth
from test_evalbatch_cpu import boundary_np, gather_np, same_dicts, score_matrix_np, tables_np

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A5A5A5A


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class Solver:
    """quber_munkres_batch on a list of cost matrices; dev_assign sits between two guard bands."""

    def __init__(self, mats, cap):
        self.mats, self.cap, B = mats, cap, len(mats)
        score = np.full((B, cap, cap), np.nan)                      # what lies outside rows x cols must not be read
        for b, m in enumerate(mats):
            score[b, :m.shape[0], :m.shape[1]] = m
        self.score = torch.from_numpy(score).cuda()
        self.rows = torch.tensor([m.shape[0] for m in mats], dtype=torch.int32, device="cuda")
        self.cols = torch.tensor([m.shape[1] for m in mats], dtype=torch.int32, device="cuda")
        self.ws = torch.empty(B * cap * cap * 8, dtype=torch.uint8, device="cuda")
        self.buf = torch.full((GUARD + B * cap + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.status = torch.full((B,), -1, dtype=torch.int32, device="cuda")

    def run(self, placement):
        lib = _lib.load()
        B = len(self.mats)
        _lib.check(lib.quber_munkres_batch(_ptr(self.score), _ptr(self.rows), _ptr(self.cols), B, self.cap, placement, _ptr(self.ws),
                                           _ptr(self.buf[GUARD:]), _ptr(self.status), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        buf = self.buf.cpu().numpy()
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "guard bytes overwritten"
        assign = buf[GUARD:-GUARD].reshape(B, self.cap)
        pairs = []
        for b, m in enumerate(self.mats):
            assert (assign[b, m.shape[0]:] == -1).all()
            pairs.append([[i, int(j)] for i, j in enumerate(assign[b, :m.shape[0]]) if j >= 0])
        return pairs, self.status.cpu().numpy()


def tie_heavy(rng, rows, cols):
    F = rng.choice([0., .25, .5, .75, 1.], (rows, cols)) * (rng.random((rows, cols)) >= 0.7)      # 70 % of the entries zeroed
    return F.max() - F


TIE_SHAPES = [(1, 1), (2, 1), (31, 33), (64, 64), (65, 64), (3, 40), (40, 3)]


@functools.lru_cache(maxsize=None)
def tie_cases():
    rng = np.random.default_rng(7)
    mats = [tie_heavy(rng, r, c) for r, c in TIE_SHAPES]
    return mats, [[list(a) for a in oracle_assign(m)] for m in mats]


def test_solver_golden_cases_in_one_batch():
    z = np.load(os.path.join(GOLDEN, "munkres_cases.npz"))
    exp = json.load(open(os.path.join(GOLDEN, "munkres_expected.json")))
    assert len(z.files) == 40
    got, status = Solver([z[k].max() - z[k] for k in z.files], 8).run(0)
    assert not status.any()
    for k, pairs in zip(z.files, got):
        assert pairs == exp[k], k


def test_solver_tie_heavy_against_oracle_in_every_placement():
    mats, exp = tie_cases()
    s = Solver(mats, 72)
    for placement in (0, 1, 2):                                      # 31 x 33 and 65 x 64 among them: LDS and device memory agree
        got, status = s.run(placement)
        assert not status.any(), (placement, status)
        for shape, g, e in zip(TIE_SHAPES, got, exp):
            assert g == e, (placement, shape)


def test_solver_beyond_the_lds_placement():
    from quber_amd.eval.assignment import munkres_assign           # equals the oracle on everything smaller (test_oracle_golden.py)
    rng = np.random.default_rng(11)
    mats = [tie_heavy(rng, 129, 129), tie_heavy(rng, 5, 4), tie_heavy(rng, 140, 120)]
    exp = [[list(a) for a in munkres_assign(m)] for m in mats]
    s = Solver(mats, 144)
    for placement in (0, 2):                                         # auto: the small frame in LDS, the large ones in the workspace
        got, status = s.run(placement)
        assert not status.any()
        assert got == exp, placement
    got, status = s.run(1)                                           # LDS forced: the frames that do not fit say so (guards checked in run)
    assert list(status) == [8, 0, 8]
    assert got[0] == [] and got[2] == [] and got[1] == exp[1]


def test_solver_second_call_overwrites_the_first():
    rng = np.random.default_rng(3)
    a = [tie_heavy(rng, 6, 9), tie_heavy(rng, 12, 12)]
    b = [tie_heavy(rng, 12, 3), tie_heavy(rng, 2, 2)]
    s = Solver(a, 12)
    first, _ = s.run(0)
    assert first == [[list(p) for p in oracle_assign(m)] for m in a]
    t = Solver(b, 12)
    t.buf, t.status, t.ws = s.buf, s.status, s.ws                   # same output buffers, other matrices
    second, status = t.run(0)
    assert second == [[list(p) for p in oracle_assign(m)] for m in b] and not status.any()
    bad = Solver([np.zeros((3, 3))], 4)
    bad.rows[0] = 5                                                  # a shape beyond cap is flagged, nothing is solved
    got, status = bad.run(0)
    assert list(status) == [2] and got == [[]]


# ------------------------------------------------------------------------------------------------ the whole call
def scene(seed, h, w, n, tricky=False):
    gtm, initm = synth.make_masks(np.random.default_rng(seed), n, h, w)
    gt, pred = np.zeros((h, w), np.int32), np.zeros((h, w), np.int32)
    for i in range(n):
        gt[gtm[i]] = i + 2
        pred[initm[i]] = i + 1
    if tricky:                                                       # the construction of test_boundary_metrics_vs_oracle
        gt[h // 3:h // 3 + 9, w // 3:w // 3 + 9] = 0                 # a hole with an object nested in it
        gt[h // 3 + 3:h // 3 + 6, w // 3 + 3:w // 3 + 6] = n + 5
        pred[:7, :] = 77                                             # an object along the frame
    return pred, gt


def check_stages(pred, gt, t, with_boundary=True):
    lp, lg, table = tables_np(pred, gt)
    assert t["status"] == 0 and not t["fallback"]
    np.testing.assert_array_equal(t["labels_pred"], lp)
    np.testing.assert_array_equal(t["labels_gt"], lg)
    np.testing.assert_array_equal(t["table"], table)
    F, cost = score_matrix_np(lp, lg, table)
    if F is None:
        assert t["F"].size == 0 and t["assignment"] == []
        return
    assert t["F"].shape == F.shape and t["F"].tobytes() == F.tobytes()          # float64 bit patterns
    assignment = oracle_assign(cost)
    assert t["assignment"] == [(i, j) for i, j in assignment]
    bnd = boundary_np(pred, gt, lp, lg) if with_boundary else (None,) * 4
    for key, want in zip(("bc_pred", "bc_gt", "ptps", "rtps"), bnd):
        if with_boundary:
            np.testing.assert_array_equal(t[key], want, err_msg=key)
        else:
            assert t[key] is None
    g = gather_np(lp, lg, table, assignment, bnd[2], bnd[3])
    for key in ("pair_tps", "pair_union") + (("pair_ptps", "pair_rtps") if with_boundary else ()):
        np.testing.assert_array_equal(t[key], g[key], err_msg=key)


def test_whole_call_mixed_batch_every_stage_and_every_dict():
    from quber_amd.eval.evaluation import multilabel_metrics, multilabel_metrics_batch
    h, w = 70, 131                                                   # tail bits; 3 words per row
    pairs = [scene(0, h, w, 3), scene(1, h, w, 6, tricky=True), scene(2, h, w, 5)]
    preds, gts = np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])
    got, tables = multilabel_metrics_batch(preds, gts, return_tables=True)
    assert len(got) == 3 and got.fallback == {}
    for (pred, gt), d, t in zip(pairs, got, tables):
        check_stages(pred, gt, t)
        same_dicts(d, multilabel_metrics(pred, gt, 0, 1, compute_boundary_stuff=True))
        same_dicts(d, metrics_np.multilabel_metrics(pred, gt, compute_boundary_stuff=True))
    assert len({len(t["labels_pred"]) for t in tables}) == 3          # different object counts side by side


@pytest.mark.parametrize("h,w", [(24, 40), (32, 128)])               # less than one word per row; whole words
def test_whole_call_other_shapes(h, w):
    from quber_amd.eval.evaluation import multilabel_metrics_batch
    pairs = [scene(5, h, w, 2), scene(6, h, w, 3)]
    got, tables = multilabel_metrics_batch(np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs]), return_tables=True)
    for (pred, gt), d, t in zip(pairs, got, tables):
        check_stages(pred, gt, t)
        same_dicts(d, metrics_np.multilabel_metrics(pred, gt, compute_boundary_stuff=True))


def test_whole_call_golden_fixtures_batched_per_shape():
    from quber_amd.eval.evaluation import multilabel_metrics, multilabel_metrics_batch
    by_shape = {}
    for path in golden("metrics"):
        z = np.load(path)
        by_shape.setdefault(z["pred"].shape, []).append((os.path.basename(path), z["pred"], z["gt"], json.loads(str(z["result"]))))
    assert sorted(len(v) for v in by_shape.values()) == [1, 1, 2, 4]
    for shape, cases in by_shape.items():
        preds, gts = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
        got = multilabel_metrics_batch(preds, gts, compute_boundary_stuff=False)
        for (name, _, _, exp), d in zip(cases, got):
            same_dicts(d, exp)
        if len(cases) == 4:                                          # frames without objects next to frames with objects, boundary stage too
            assert sorted(c[0] for c in cases) == ["metrics_disjoint.npz", "metrics_none_both.npz", "metrics_none_gt.npz", "metrics_none_pred.npz"]
            got, tables = multilabel_metrics_batch(preds, gts, return_tables=True)
            for (name, pred, gt, _), d, t in zip(cases, got, tables):
                check_stages(pred, gt, t)
                same_dicts(d, multilabel_metrics(pred, gt, 0, 1, compute_boundary_stuff=True))


def test_labels_and_cap():
    from quber_amd.eval.evaluation import multilabel_metrics, multilabel_metrics_batch
    h, w = 40, 70
    pred, gt = scene(8, h, w, 2)
    wide = np.where(pred == 1, 7, np.where(pred == 2, 65535, 0)).astype(np.int32)          # labels {0, 7, 65535}
    full = (np.arange(h * w).reshape(h, w) // (h * w // 3 + 1) + 1).astype(np.int32)      # no background at all
    many = (np.arange(h * w).reshape(h, w) % 17).astype(np.int32)                           # 17 labels
    preds, gts = np.stack([wide, full, pred, many]), np.stack([gt, gt, full, gt])
    got, tables = multilabel_metrics_batch(preds, gts, cap=16, return_tables=True)
    assert got.fallback == {3: 2} and tables[3] == {"status": 2, "fallback": True}          # flagged, never truncated
    for b in range(4):
        same_dicts(got[b], multilabel_metrics(preds[b], gts[b], 0, 1, compute_boundary_stuff=True))
        if b < 3:
            check_stages(preds[b], gts[b], tables[b])
    np.testing.assert_array_equal(tables[0]["labels_pred"], [0, 7, 65535])
    assert tables[1]["labels_pred"][0] != 0 and tables[2]["labels_gt"][0] != 0
    # a label of -1: numpy input is renumbered on the host (the per-frame path), device input is refused
    void = pred.astype(np.int64)
    void[:5] = -1
    got = multilabel_metrics_batch(np.stack([void, pred]), np.stack([gt, gt]))
    assert got.fallback == {0: 1}
    same_dicts(got[0], multilabel_metrics(void, gt, 0, 1, compute_boundary_stuff=True))
    same_dicts(got[1], multilabel_metrics(pred, gt, 0, 1, compute_boundary_stuff=True))
    with pytest.raises(ValueError):
        multilabel_metrics_batch(torch.from_numpy(np.stack([void, pred]).astype(np.int32)).cuda(), torch.from_numpy(np.stack([gt, gt])).cuda())
    big = np.stack([pred.astype(np.int64) * (2 ** 32 + 1)])                                  # must not alias 0..65535 through int32
    same_dicts(multilabel_metrics_batch(big, np.stack([gt]))[0], multilabel_metrics(pred, gt, 0, 1, compute_boundary_stuff=True))


def test_without_boundary_and_two_handles_in_flight():
    from quber_amd.eval.evaluation import collect_metrics, enqueue_metrics, multilabel_metrics, multilabel_metrics_batch
    lib = _lib.load()
    h, w = 70, 131
    a, b = scene(0, h, w, 3), scene(1, h, w, 6, tricky=True)
    # no boundary work: no planes in the workspace, None for the boundary keys, as the per-frame function
    assert lib.quber_eval_batch_workspace_bytes(2, h, w, 64, 0) == 2 * (786440 + 16 * 64 * 64)
    assert lib.quber_eval_batch_workspace_bytes(2, h, w, 64, 1) == 2 * (786440 + 16 * 64 * 64 + 3 * 128 * h * 3 * 8)
    got, tables = multilabel_metrics_batch(np.stack([a[0], b[0]]), np.stack([a[1], b[1]]), compute_boundary_stuff=False, return_tables=True)
    for (pred, gt), d, t in zip((a, b), got, tables):
        assert d["Boundary F-measure"] is None and d["Boundary OSN Recall"] is None
        check_stages(pred, gt, t, with_boundary=False)
        same_dicts(d, multilabel_metrics(pred, gt, 0, 1, compute_boundary_stuff=False))
    # two handles of one shape enqueued before either is collected: device tensors in, each handle keeps its own results
    dev = lambda x: torch.from_numpy(np.stack(x)).cuda()
    h1 = enqueue_metrics(dev([a[0], b[0]]), dev([a[1], b[1]]))
    h2 = enqueue_metrics(dev([b[0], a[0]]), dev([a[1], b[1]]))
    r1, r2 = collect_metrics(h1), collect_metrics(h2)
    for d, (pred, gt) in zip(r1 + r2, [(a[0], a[1]), (b[0], b[1]), (b[0], a[1]), (a[0], b[1])]):
        same_dicts(d, multilabel_metrics(pred, gt, 0, 1, compute_boundary_stuff=True))


def test_evaluate_stream_equals_per_frame_metrics(tmp_path):
    from PIL import Image
    from quber_amd import arch
    from quber_amd.eval.evaluation import multilabel_metrics
    from quber_amd.eval.refiner_model import MaskRefiner, label_map_from_masks
    items, annos = [], []
    for i in range(3):
        sc = synth.make_scene(60 + i, 480, 640, 4)
        Image.fromarray(sc["rgb"][:, :, ::-1].copy()).save(tmp_path / f"rgb{i}.png")
        Image.fromarray(sc["depth"][:, :, 0].astype(np.uint16) * 5 + 300).save(tmp_path / f"depth{i}.png")
        anno = label_map_from_masks(sc["gt_masks"], (480, 640), np.uint8)
        Image.fromarray(anno).save(tmp_path / f"anno{i}.png")
        items.append((str(tmp_path / f"rgb{i}.png"), str(tmp_path / f"depth{i}.png"), sc["masks"] != 0, None))
        annos.append((str(tmp_path / f"anno{i}.png"), anno))
    ref = MaskRefiner(None, None, dataset="OSD")
    model = ref.refiner_predictor.model                              # random weights with loud heads: real instances come out
    model.state_dict = arch.init_state_dict(seed=0, loud_heads=True, center_bias=-1.68)
    model._engines.clear()
    got = list(ref.evaluate_stream(items, [p for p, _ in annos], workers=2, batch=2))              # 2 + 1 frames
    assert len(got) == 3 and sum(len(r[0]) for r in got) >= 3
    for (refined, output, secs, fg, initial_metrics, refined_metrics), item, (_, anno) in zip(got, items, annos):
        assert "sem_seg" in output and secs > 0
        same_dicts(initial_metrics, multilabel_metrics(label_map_from_masks(item[2], anno.shape), anno, 1, 1))
        same_dicts(refined_metrics, multilabel_metrics(label_map_from_masks(refined, anno.shape), anno, 1, 1))
