"""GPU: the mean-shift clustering of pixel embeddings on the device (csrc/meanshift.hip through Engine.meanshift_* and
MaskRefinerPredictor(cluster=...)) against its numpy contract (tests/test_meanshift_cpu.py).  Every stage is fed the contract's own
inputs.  Seeds, link, assign, filter and compaction are compared bit for bit; the climb against the float64 statement, with a bar the
test derives from the error of torch's own float32 mm / exp on the same inputs (4 x that error: the room is for the tiled summation
order and the hardware exp; a dropped or doubled tile of pixels moves a mode by about 1e-3)."""
import numpy as np
import pytest
import torch

from quber_amd import engine
from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
from quber_amd.meanshift import MeanShift
from quber_amd.perturb import Perturb
from test_meanshift_cpu import (CHANNELS, assign_np, blob_embeddings, chain_cases, climb_np, cluster_np, decidable, filter_depth_np, grid_embeddings,
                                hand_cases, link_np, meanshift_np, seeds_np)

pytestmark = pytest.mark.gpu

# fewer pixels than a persistent grid has blocks of tiles; odd rows, a partial last tile, unaligned stores; whole tiles
SHAPES = [(24, 32), (37, 53), (48, 64)]
SEEDS = [1, 2, 31, 32, 33, 100, 128]           # below, at and above the 32-row MFMA tile; the reference's; the padded maximum
B = 3
N_MASKS = 6
FILL = 0x3C


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_ENGINES = {}


def _engine(h, w, batch=B, cap=64):
    key = (h, w, batch, cap)
    if key not in _ENGINES:
        _ENGINES[key] = engine.Engine(engine.make_config(h, w, max_batch=batch, max_instances=cap, with_network=False), "cuda:0")
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    torch.cuda.synchronize()
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def guarded(shape, dtype, shift=3):
    """A tensor `shift` elements into a buffer filled with a sentinel byte -> (view, check())."""
    n, es = int(np.prod(shape)), torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((shift + n + 64) * es,), FILL, dtype=torch.uint8, device="cuda")
    view = raw.view(dtype)[shift:shift + n].view(shape)
    intact = lambda: bool((raw[:shift * es] == FILL).all()) and bool((raw[(shift + n) * es:] == FILL).all())
    return view, intact


_FRAMES = {}


def frames(h, w):
    """B frames of one shape: two blob frames (4 and 5 clusters) and a grid frame, their first seeds, and a depth plane each that starves
    cluster 1 of depth.  -> (emb f32 [B,64,h,w], first i32 [B], depth_z f32 [B,h,w], which)"""
    if (h, w) not in _FRAMES:
        made = [blob_embeddings(h, w, 4, 21), blob_embeddings(h, w, 5, 22), grid_embeddings(h, w, 4, 23)]
        emb, which = np.stack([m[0] for m in made]), np.stack([m[1] for m in made])
        first = np.array([5, h * w - 1, h * w // 2], np.int32)
        rng = np.random.RandomState(h)
        z = np.where((which == 1) & (rng.rand(B, h, w) < 0.75), 0, 1).astype(np.float32)
        _FRAMES[(h, w)] = (emb, first, z, which)
    return _FRAMES[(h, w)]


def rows(emb):
    return emb.reshape(CHANNELS, -1).T


_CONTRACT = {}


def contract(h, w, S):
    """meanshift_np of the B frames of a shape with S seeds, computed once."""
    if (h, w, S) not in _CONTRACT:
        emb, first, _, _ = frames(h, w)
        _CONTRACT[(h, w, S)] = [meanshift_np(rows(emb[b]), int(first[b]), S) for b in range(B)]
    return _CONTRACT[(h, w, S)]


@pytest.mark.parametrize("S", SEEDS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_seeds_equal_contract(h, w, S):
    emb, first, _, _ = frames(h, w)
    out, intact = guarded((B, S), torch.int32)
    _engine(h, w).meanshift_seeds(dev(emb), dev(first), S, out=out)
    torch.cuda.synchronize()
    want = np.stack([seeds_np(rows(emb[b]), int(first[b]), S) for b in range(B)]) if S != 100 else np.stack([c["indices"] for c in contract(h, w, S)])
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert intact()


def test_seeds_ties_and_negative_distances():
    """All pixels identical (every step a full tie: index 0 wins) and rows longer than 1 (negative distances order correctly)."""
    h, w = SHAPES[1]
    rng = np.random.RandomState(3)
    same = np.broadcast_to((rng.randint(-8, 9, CHANNELS) / 64.0).astype(np.float32)[:, None, None], (CHANNELS, h, w))
    long = (rng.randint(-16, 17, (CHANNELS, h, w)) / 16.0).astype(np.float32)
    emb = np.ascontiguousarray(np.stack([same, long, long[:, ::-1]]))
    first = np.array([7, 0, 11], np.int32)
    got = _engine(h, w).meanshift_seeds(dev(emb), dev(first), 9).cpu().numpy()
    want = np.stack([seeds_np(rows(emb[b]), int(first[b]), 9) for b in range(B)])
    np.testing.assert_array_equal(got, want)
    assert got[0].tolist() == [7] + [0] * 8


@pytest.mark.parametrize("S", SEEDS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_climb_within_the_bar_and_bit_equal(h, w, S):
    """Against the float64 statement on the same float32 inputs.  The bar: 4 x the error of torch's float32 mm / exp on the CPU."""
    emb, first, _, _ = frames(h, w)
    idx = np.stack([seeds_np(rows(emb[b]), int(first[b]), S) for b in range(B)]) if S != 100 else np.stack([c["indices"] for c in contract(h, w, S)])
    want = np.stack([climb_np(rows(emb[b]), rows(emb[b])[idx[b]], 20.0, 10) for b in range(B)])
    e_ref = 0.0
    for b in range(B):
        X = torch.from_numpy(rows(emb[b]).copy())
        Z = X[torch.from_numpy(idx[b].astype(np.int64))]
        for _ in range(10):
            Z = torch.nn.functional.normalize(torch.mm(torch.exp(20.0 * torch.mm(Z, X.t())), X), p=2, dim=1)
        e_ref = max(e_ref, float(np.abs(Z.numpy().astype(np.float64) - want[b]).max()))
    eng = _engine(h, w)
    out, intact = guarded((B, S, CHANNELS), torch.float32)
    eng.meanshift_climb(dev(emb), seeds=out, indices=dev(idx))
    again = eng.meanshift_climb(dev(emb), indices=dev(idx))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"climb {h}x{w} S={S}: device error {err:.3e}, torch float32 error e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}")
    assert intact(), "wrote outside the seeds (a padded seed row reached the output)"
    assert np.array_equal(got.view(np.uint32), again.cpu().numpy().view(np.uint32)), "two runs differ"
    assert err <= 4 * e_ref, (err, e_ref)
    # started from its contents (no indices) it does the same
    z0 = dev(np.stack([rows(emb[b])[idx[b]] for b in range(B)]))
    assert torch.equal(eng.meanshift_climb(dev(emb), seeds=z0), out)


def _stage_inputs(h, w, S):
    emb, first, z, _ = frames(h, w)
    c = contract(h, w, S)
    return emb, z, np.stack([r["seeds"] for r in c]), np.stack([r["seed_labels"] for r in c])


@pytest.mark.parametrize("S", [2, 33, 100, 128])
@pytest.mark.parametrize("h,w", SHAPES)
def test_link_and_assign_equal_contract_on_recorded_seeds(h, w, S):
    emb, z, Z, sl = _stage_inputs(h, w, S)
    eng = _engine(h, w)
    labels, ok = guarded((B, S), torch.int32)
    eng.meanshift_link(dev(Z), 0.04, out=labels)
    np.testing.assert_array_equal(labels.cpu().numpy(), sl)
    assert ok()
    for depth, thr in ((None, None), (z, 0.5), (z, 0.1)):
        ids, ok1 = guarded((B, h, w), torch.int32, shift=1 if depth is None else 4)     # unaligned, then 16-byte aligned: both store forms
        masks, ok2 = guarded((B, N_MASKS, h, w), torch.uint8, shift=1 if depth is None else 16)
        rep, ok3 = guarded((B, 4), torch.int32)
        eng.meanshift_assign(dev(emb), dev(Z), dev(sl), N_MASKS, None if depth is None else dev(depth), thr, ids, masks, rep)
        torch.cuda.synchronize()
        for b in range(B):
            lab = assign_np(rows(emb[b]), Z[b], sl[b])[1]
            want, wrep = filter_depth_np(lab, None if depth is None else depth[b].reshape(-1), thr, N_MASKS)
            np.testing.assert_array_equal(ids[b].cpu().numpy().reshape(-1), want)
            np.testing.assert_array_equal(rep[b].cpu().numpy(), wrep)
            np.testing.assert_array_equal(masks[b].cpu().numpy().reshape(N_MASKS, -1), np.stack([(want == k + 1) * 255 for k in range(N_MASKS)]))
        assert ok1() and ok2() and ok3()
    if S >= 33:
        assert rep[:, 2].sum() == 0 and rep[:, 0].tolist() == [3, 4, 3]          # at 0.1 nothing is dropped; at 0.5 (checked above) cluster 1 is


def test_truncation_to_the_planes_there_are():
    h, w = SHAPES[0]
    emb, z, Z, sl = _stage_inputs(h, w, 33)
    r = _engine(h, w).meanshift_assign(dev(emb), dev(Z), dev(sl), 2)
    for b in range(B):
        want, wrep = filter_depth_np(assign_np(rows(emb[b]), Z[b], sl[b])[1], max_masks=2)
        np.testing.assert_array_equal(r["ids"][b].cpu().numpy().reshape(-1), want)
        assert r["report"][b].tolist() == wrep.tolist() and wrep[3] == 1 and want.max() == 2


@pytest.mark.parametrize("name,h,w", [("vanishing_label", 2, 7), ("one_cluster", 3, 4), ("all_identical", 1, 17), ("depth_drops_one", 5, 7),
                                      ("chain_mode", 2, 7), ("chain_tie", 2, 7), ("chain_tie_order", 2, 7), ("chain_vanish", 2, 7)])
def test_hand_cases(name, h, w):
    Z, X, z, thr = hand_cases()[name]
    eng = _engine(h, w, 1)
    emb = np.ascontiguousarray(X.T.reshape(1, CHANNELS, h, w))
    sl = eng.meanshift_link(dev(Z[None]), 0.04)
    want_sl = link_np(Z, 0.04)
    np.testing.assert_array_equal(sl[0].cpu().numpy(), want_sl)
    if name.startswith("chain_"):                            # the mode branch of the labelling: the labels the CPU test asserts literally
        assert want_sl.tolist() == chain_cases()[name][1]
    r = eng.meanshift_assign(dev(emb), dev(Z[None]), sl, 4, None if z is None else dev(z.reshape(1, h, w)), thr)
    want, wrep = filter_depth_np(assign_np(X, Z, want_sl)[1], z, thr, 4)
    np.testing.assert_array_equal(r["ids"][0].cpu().numpy().reshape(-1), want)
    assert r["report"][0].tolist() == wrep.tolist()
    if name in ("one_cluster", "all_identical"):
        assert wrep[0] == 0 and not r["masks"].any()


@pytest.mark.parametrize("S", [33, 100, 128])
@pytest.mark.parametrize("h,w", SHAPES)
def test_chain_equals_contract(h, w, S):
    emb, first, z, _ = frames(h, w)
    ms = MeanShift(num_seeds=S, depth_threshold=0.5)
    want = [cluster_np(emb[b], int(first[b]), ms, z[b], N_MASKS) for b in range(B)]
    for b in range(B):                                       # the input is decidable: the device's float32 climb cannot change a label
        assert decidable(rows(emb[b]), want[b]["seeds"], want[b]["seed_labels"], ms.epsilon)
    shapes = {"indices": ((B, S), torch.int32), "seeds": ((B, S, CHANNELS), torch.float32), "seed_labels": ((B, S), torch.int32),
              "ids": ((B, h, w), torch.int32), "masks": ((B, N_MASKS, h, w), torch.uint8), "report": ((B, 4), torch.int32)}
    out, checks = {}, []
    for k, (shape, dtype) in shapes.items():
        out[k], ok = guarded(shape, dtype, shift=1 if k in ("ids", "masks") else 3)
        checks.append(ok)
    eng = _engine(h, w)
    # a first call on other frames (the batch reversed, no depth filter) fills every output; the second must overwrite all of it
    eng.meanshift(dev(emb[::-1]), dev(first[::-1]), MeanShift(num_seeds=S), N_MASKS, out=out)
    r = eng.meanshift(dev(emb), dev(first), ms, N_MASKS, dev(z), out=out)
    torch.cuda.synchronize()
    assert all(r[k].data_ptr() == out[k].data_ptr() for k in out) and all(ok() for ok in checks)
    for b in range(B):
        for k in ("indices", "seed_labels", "ids", "masks", "report"):
            np.testing.assert_array_equal(r[k][b].cpu().numpy(), want[b][k], err_msg=f"frame {b}: {k}")
        assert np.abs(r["seeds"][b].cpu().numpy() - want[b]["seeds"]).max() < 1e-5
        ids = r["ids"][b].cpu().numpy()
        assert ((r["masks"][b].cpu().numpy() != 0).sum(axis=0) == (ids != 0)).all()          # no pixel left out, none twice
    assert [w_["report"].tolist() for w_ in want] == [[2, 3, 1, 0], [3, 4, 1, 0], [2, 3, 1, 0]]
    # a frame's result does not depend on the batch it is in
    alone = eng.meanshift(dev(emb[1:2]), dev(first[1:2]), ms, N_MASKS, dev(z[1:2]))
    assert all(torch.equal(alone[k][0], r[k][1]) for k in out)


@pytest.mark.parametrize("name", ["meanshift_grid_24x32.npz", "meanshift_blob_24x32.npz", "meanshift_grid_37x53.npz", "meanshift_blob_37x53.npz"])
def test_chain_on_the_reference_fixtures(name):
    """The chain on the inputs the fixtures were recorded on, against what the reference's own functions returned: on grid inputs the
    seed indices, seed labels and the filtered, renumbered label map exactly; on blob inputs the label map as a partition."""
    import os
    from test_meanshift_cpu import GOLDEN, same_partition
    g = np.load(os.path.join(GOLDEN, name))
    emb = g["emb"].astype(np.float32)
    h, w = emb.shape[1:]
    ms = MeanShift(num_seeds=int(g["num_seeds"]), kappa=float(g["kappa"]), iters=int(g["iters"]), alpha=0.02, depth_threshold=float(g["threshold"]))
    r = _engine(h, w, 1).meanshift(dev(emb[None]), dev(g["indices"][:1].astype(np.int32)), ms, N_MASKS, dev(g["depth_z"][None]))
    ids = r["ids"][0].cpu().numpy()
    if "grid" in name:
        np.testing.assert_array_equal(r["indices"][0].cpu().numpy(), g["indices"])
        np.testing.assert_array_equal(r["seed_labels"][0].cpu().numpy(), g["seed_labels"])
        np.testing.assert_array_equal(ids, g["filtered"])
        assert np.abs(r["seeds"][0].cpu().numpy().astype(np.float64) - g["seeds"]).max() < 1e-5      # (the reference climbs in float32)
    else:
        assert same_partition(ids, g["filtered"])
    assert int(r["report"][0, 0]) == int(g["filtered"].max()) and int(r["report"][0, 2]) >= 1


def test_bad_arguments_are_refused_and_launch_nothing():
    h, w = SHAPES[0]
    eng = _engine(h, w, B, 32)
    emb, first, z, _ = frames(h, w)
    d_emb, d_first, d_z = dev(emb), dev(first), dev(z)
    P, st = engine._ptr, engine._stream
    bufs = {k: guarded(s, t) for k, (s, t) in {"idx": ((B, 128), torch.int32), "seeds": ((B, 128, CHANNELS), torch.float32),
                                               "sl": ((B, 128), torch.int32), "ids": ((B, h, w), torch.int32),
                                               "masks": ((B, 4, h, w), torch.uint8), "rep": ((B, 4), torch.int32)}.items()}
    v = {k: b[0] for k, b in bufs.items()}
    lib, H = eng.lib, eng.h
    before = lib.quber_workspace_bytes(H)
    err = lambda: lib.quber_last_error()
    assert lib.quber_meanshift_seeds(H, P(d_emb), B, 32, P(d_first), 8, P(v["idx"]), st()) != 0 and b"64 channels" in err()
    assert lib.quber_meanshift_seeds(H, P(d_emb), B, 64, P(d_first), 129, P(v["idx"]), st()) != 0 and b"num_seeds" in err()
    assert lib.quber_meanshift_seeds(H, P(d_emb), B, 64, P(d_first), 0, P(v["idx"]), st()) != 0
    assert lib.quber_meanshift_seeds(H, P(d_emb), B + 1, 64, P(d_first), 8, P(v["idx"]), st()) != 0
    assert lib.quber_meanshift_seeds(H, None, B, 64, P(d_first), 8, P(v["idx"]), st()) != 0 and b"null" in err()
    assert lib.quber_meanshift_seeds(H, P(d_emb), B, 64, None, 8, P(v["idx"]), st()) != 0
    assert lib.quber_meanshift_climb(H, P(d_emb), B, 64, None, 8, 20.0, -1, P(v["seeds"]), st()) != 0 and b"iters" in err()
    assert lib.quber_meanshift_climb(H, P(d_emb), B, 64, None, 8, float("nan"), 10, P(v["seeds"]), st()) != 0 and b"kappa" in err()
    assert lib.quber_meanshift_climb(H, P(d_emb), B, 64, None, 8, 64.5, 10, P(v["seeds"]), st()) != 0 and b"kappa" in err()
    assert lib.quber_meanshift_climb(H, P(d_emb), B, 64, None, 8, 20.0, 10, None, st()) != 0
    assert lib.quber_meanshift_link(H, P(v["seeds"]), B, 129, 0.04, P(v["sl"]), st()) != 0
    assert lib.quber_meanshift_link(H, P(v["seeds"]), B, 8, -1.0, P(v["sl"]), st()) != 0 and b"epsilon" in err()
    assert lib.quber_meanshift_assign(H, P(d_emb), B, 64, P(v["seeds"]), P(v["sl"]), 8, P(d_z), 1.5, 4, P(v["ids"]), P(v["masks"]), P(v["rep"]), st()) != 0
    assert lib.quber_meanshift_assign(H, P(d_emb), B, 64, P(v["seeds"]), P(v["sl"]), 8, None, 0.0, 255, P(v["ids"]), P(v["masks"]), P(v["rep"]), st()) != 0
    assert lib.quber_meanshift_assign(H, P(d_emb), B, 64, P(v["seeds"]), P(v["sl"]), 8, None, 0.0, 4, P(v["ids"]), None, P(v["rep"]), st()) != 0
    args = lambda **kw: [kw.get("emb", P(d_emb)), B, kw.get("c", 64), P(d_first), kw.get("S", 8), 20.0, 10, 0.04, None, 0.0, 4, P(v["idx"]), P(v["seeds"]),
                         P(v["sl"]), P(v["ids"]), kw.get("masks", P(v["masks"])), P(v["rep"]), st()]
    assert lib.quber_meanshift_cluster(H, *args(c=63)) != 0 and b"64 channels" in err()
    assert lib.quber_meanshift_cluster(H, *args(S=200)) != 0
    assert lib.quber_meanshift_cluster(H, *args(masks=None)) != 0
    tiny = _engine(2, 3, 1)
    assert tiny.lib.quber_meanshift_seeds(tiny.h, P(d_emb), 1, 64, P(d_first), 7, P(v["idx"]), st()) != 0 and b"more seeds" in err()
    big = _engine(4097, 4096, 1, 1)
    assert big.lib.quber_meanshift_seeds(big.h, P(d_emb), 1, 64, P(d_first), 7, P(v["idx"]), st()) != 0 and b"2^24" in err()
    torch.cuda.synchronize()
    assert all(b[1]() for b in bufs.values()) and all(bool((x.view(-1).view(torch.uint8) == FILL).all()) for x in v.values()), "a refused call wrote"
    # a context that never clusters holds no workspace for it; the first good call allocates it, later ones nothing
    assert lib.quber_workspace_bytes(H) == before, "a refused call allocated"
    eng.meanshift_link(dev(np.zeros((B, 4, CHANNELS), np.float32)))
    assert lib.quber_workspace_bytes(H) == before                # (the link needs no workspace)
    eng.meanshift(d_emb, d_first, MeanShift(num_seeds=8), 4)
    after = lib.quber_workspace_bytes(H)
    eng.meanshift(d_emb, d_first, MeanShift(num_seeds=128), 4)
    assert after > before and lib.quber_workspace_bytes(H) == after


# ---- end to end ----
CLUSTER_KEYS = {"cluster_masks", "cluster_ids", "cluster_seeds", "cluster_report"}


@pytest.mark.parametrize("variant", ["plain", "perturb"])
def test_predictor_cluster_equals_none_fed_with_the_contract(variant):
    """MaskRefinerPredictor(cluster=MeanShift(...)) on embeddings = the same predictor without cluster fed the contract's masks, in every
    output key; with perturb= set as well the perturbation acts on the clustering's masks (one walk for all masks - a seed that
    broadcasts - because the two predictors run it on different numbers of planes)."""
    from quber_amd import synth
    from test_gpu_cleanup import speck_logits
    from test_gpu_masknms import _equal, _predictor
    h, w = 96, 128
    logits = speck_logits(h, w)
    sc = [synth.make_scene(3 + b, h, w, 2) for b in range(2)]
    rgb, dep = np.stack([s["rgb"] for s in sc]), np.stack([s["depth"] for s in sc])
    made = [blob_embeddings(h, w, 4, 31), blob_embeddings(h, w, 6, 32)]
    emb = [m[0] for m in made]
    if variant == "plain":
        ms = MeanShift(num_seeds=33, depth_threshold=0.5, seed=5)
        z = [np.where(m[1] == 2, 0, 1).astype(np.float32) for m in made]        # cluster 2 has no depth at all
        kw = dict(decode_errors=True, track_initial=True, tta=True, iterations=2)
    else:
        ms, z = MeanShift(num_seeds=33, seed=5), None
        kw = dict(decode_errors=True, perturb=Perturb(0.8, seeds=np.array([[3]]), rounds=20))
    first = np.random.RandomState(5).randint(0, h * w, 3)                       # one draw per frame, in frame order: two calls, three frames
    want = [cluster_np(emb[b], int(first[b]), ms, None if z is None else z[b], 32) for b in range(2)]
    want.append(cluster_np(emb[1], int(first[2]), ms, None if z is None else z[1], 32))
    for b, r in enumerate(want):
        assert decidable(rows(emb[min(b, 1)]), r["seeds"], r["seed_labels"], ms.epsilon)
    counts = [int(r["report"][0]) for r in want]
    assert counts == ([2, 4, 4] if variant == "plain" else [3, 5, 5])
    fed = [r["masks"][:c] for r, c in zip(want, counts)]
    got_off, want_off = [], []
    with_cluster = _predictor(h, w, logits, got_off, cluster=ms, **kw)
    none = _predictor(h, w, logits, want_off, **kw)

    def check(a, b, f, what):
        assert set(a) - CLUSTER_KEYS == set(b) and CLUSTER_KEYS <= set(a) and not CLUSTER_KEYS & set(b), (what, sorted(a), sorted(b))
        for key in b:
            _equal(a[key], b[key], "%s frame %d: %s" % (what, f, key))
        r = want[f]
        np.testing.assert_array_equal(a["cluster_masks"].cpu().numpy(), fed[f])
        np.testing.assert_array_equal(a["cluster_ids"].cpu().numpy(), r["ids"])
        assert a["cluster_report"].dtype == torch.int64 and a["cluster_report"].tolist() == r["report"].tolist()
        assert np.abs(a["cluster_seeds"].cpu().numpy() - r["seeds"]).max() < 1e-5

    outs = with_cluster.predict_batch(rgb, dep, None, embeddings=emb, depth_z=z)
    refs = none.predict_batch(rgb, dep, fed[:2])
    for f, (a, b) in enumerate(zip(outs, refs)):
        check(a, b, f, "predict_batch")
    if variant == "perturb":
        assert not np.array_equal(outs[0]["perturbed_masks"].cpu().numpy(), fed[0])          # the walk did something - to the clustering's masks
    a = with_cluster.predict(rgb[1], dep[1], embeddings=emb[1], depth_z=None if z is None else z[1])[0]      # one frame: the third draw
    b = none.predict_batch(rgb[1:], dep[1:], fed[2:])[0]
    check(a, b, 2, "predict")
    assert len(got_off) == len(want_off) >= 2
    for x, y in zip(got_off, want_off):
        assert x.shape == y.shape and torch.equal(x, y)
    with pytest.raises(ValueError):
        with_cluster.predict_batch(rgb, dep, fed[:2], embeddings=emb)                       # masks and embeddings
    with pytest.raises(ValueError):
        with_cluster.predict_batch(rgb, dep, None)                                          # no embeddings
    with pytest.raises(ValueError):
        with_cluster.predict(rgb[0], dep[0], fed[0])
    with pytest.raises(ValueError):
        with_cluster.predict(rgb[0], dep[0], mask_scores=np.ones(2, np.float32), embeddings=emb[0])      # scores with nothing to score
    with pytest.raises(ValueError):
        none.predict_batch(rgb, dep, fed[:2], embeddings=emb)                               # embeddings without cluster=
    with pytest.raises(ValueError):
        with_cluster.model.enqueue_batch(dev(rgb), dev(dep), dev(np.zeros((2, 1, h, w), np.uint8)))
    if variant == "plain":
        with pytest.raises(ValueError):
            with_cluster.predict_batch(rgb, dep, None, embeddings=emb)                      # depth_threshold without depth_z
    with_cluster.model.close()
    none.model.close()
