"""GPU: the Gaussian mean shift of centre votes and the IMP on the device (csrc/gms.hip through Engine.gms_* and
MaskRefinerPredictor(cluster=GaussianMeanShift(...))) against the numpy contract (tests/test_gms_cpu.py).  Every stage is fed the
contract's own inputs.  Seeds, link, assign, filter, renumbering, centres and the IMP are compared bit for bit; the climb against the
float64 statement, with the bar 4 x max(e_ref, one float32 ulp of the largest |coordinate| of the frame), e_ref being the error of the
reference's formula restated in float32 torch on the CPU (4 is the project's bar for the UCN climb; the ulp floor because e_ref can land
on the output's own rounding).  Ratios measured on an MI355X: profiles/gms_ab.md."""
import os

import numpy as np
import pytest
import torch

from quber_amd import engine
from quber_amd.gms import IMP, GaussianMeanShift
from test_gms_cpu import (FIXTURES, GOLDEN, assign_np, climb_np, compact_np, decidable, filter_np, fixture_options, gms_np, imp_np, link_np,
                          same_partition, seeds_np, small_options, vote_scene, voronoi_map)

pytestmark = pytest.mark.gpu

# a frame smaller than one compaction block; odd, with n not a multiple of subsample; W not a multiple of 32, several blocks
SHAPES = [(24, 32), (37, 53), (61, 83)]
B = 3
N_MASKS = 8
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


_BATCHES = {}


def batch(h, w, seed=0):
    """Three frames with different foreground counts - a scene with strays, NO foreground, fewer subsampled points than seeds - their
    draws, and the contract of each.  Computed once per shape and never changed."""
    key = (h, w, seed)
    if key not in _BATCHES:
        g = small_options()
        votes, fg = [], []
        for b in range(B):
            v, f, _ = vote_scene(h, w, 3 + (b + seed) % 2, seed=10 * seed + b + h, stray=3)
            votes.append(v)
            fg.append(f)
        fg[1] = np.zeros_like(fg[1])
        few = np.zeros_like(fg[2])
        on = np.flatnonzero(fg[2])
        few.reshape(-1)[on[np.linspace(0, len(on) - 1, 93).astype(int)]] = 1                      # n = 93: n_sub = 19 < 40 seeds
        fg[2] = few
        votes, fg = np.stack(votes), np.stack(fg)
        first, draws = GaussianMeanShift(num_seeds=g.num_seeds, seed=7 + seed).draws([g.n_sub(int(f.sum())) for f in fg])
        want = [gms_np(votes[b], fg[b], first[b], draws[b], small_options(min_pixels=20 if b != 2 else 5), N_MASKS) for b in range(B)]
        assert want[1]["info"].tolist() == [0, 0, 0] and want[2]["info"].tolist() == [93, 19, 19] and want[0]["info"][2] == 40
        assert int(fg[0].sum()) % g.subsample != 0 or (h, w) != (37, 53)
        _BATCHES[key] = (votes, fg, first, draws, want)
    return _BATCHES[key]


def padded(rows, S, fill, width=None):
    out = np.full((len(rows), S) + (() if width is None else (width,)), fill, rows[0].dtype)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def e_ref(Xs, Z0, sigma, iters):
    """The reference's formula (cluster.py: gaussian_kernel, seed_hill_climbing) restated in float32 torch on the CPU."""
    X, Z = torch.from_numpy(np.ascontiguousarray(Xs, np.float32)), torch.from_numpy(np.ascontiguousarray(Z0, np.float32))
    for _ in range(iters):
        W = torch.exp(-.5 / (sigma ** 2) * torch.norm(Z.unsqueeze(1) - X.unsqueeze(0), dim=2) ** 2)
        Z = torch.mm(W / W.sum(dim=1, keepdim=True), X)
    return Z.numpy()


@pytest.mark.parametrize("h,w", SHAPES)
def test_stages_equal_contract(h, w):
    votes, fg, first, draws, want = batch(h, w)
    g = small_options()
    eng = _engine(h, w)
    S = g.num_seeds
    d_votes, d_fg = dev(votes), dev(fg)
    # seeds
    idx, ok1 = guarded((B, S), torch.int32)
    info, ok2 = guarded((B, 3), torch.int32)
    eng.gms_seeds(d_votes, d_fg, dev(first), dev(draws.view(np.int32)), g.subsample, out=idx, info=info)
    np.testing.assert_array_equal(idx.cpu().numpy(), padded([r["indices"] for r in want], S, -1))
    np.testing.assert_array_equal(info.cpu().numpy(), np.stack([r["info"] for r in want]))
    # climb, from the contract's indices: the bar, and two calls give equal bits
    Z, ok3 = guarded((B, S, 3), torch.float32)
    eng.gms_climb(d_votes, d_fg, seeds=Z, indices=idx, info=info, sigma=g.sigma, iters=g.iters, subsample=g.subsample)
    got = Z.cpu().numpy()
    again = eng.gms_climb(d_votes, d_fg, indices=idx, info=info, sigma=g.sigma, iters=g.iters, subsample=g.subsample).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    for b, r in enumerate(want):
        s = len(r["indices"])
        assert not got[b, s:].any()
        if not s:
            continue
        _, Xs = compact_np(votes[b], fg[b], g.subsample)
        exact = climb_np(Xs, Xs[r["indices"]], g.sigma, g.iters)
        ref = np.abs(e_ref(Xs, Xs[r["indices"]], g.sigma, g.iters).astype(np.float64) - exact).max()
        ulp = float(np.spacing(np.float32(np.abs(Xs).max())))
        err = np.abs(got[b, :s].astype(np.float64) - exact).max()
        print("climb %dx%d frame %d: err %.3e, e_ref %.3e, ulp %.3e, ratio %.3f" % (h, w, b, err, ref, ulp, err / max(ref, ulp)))
        assert err <= 4 * max(ref, ulp), (b, err, ref, ulp)
    # link and assign on the contract's climbed seeds
    Zc = dev(padded([r["seeds"] for r in want], S, 0, 3))
    lab, ok4 = guarded((B, S), torch.int32)
    eng.gms_link(Zc, info, g.epsilon, out=lab)
    np.testing.assert_array_equal(lab.cpu().numpy(), padded([r["seed_labels"] for r in want], S, -1))
    for min_pixels, rows in ((20, (0, 1)), (5, (2,))):
        ids, ok5 = guarded((B, h, w), torch.int32)
        masks, ok6 = guarded((B, N_MASKS, h, w), torch.uint8)
        cen, ok7 = guarded((B, N_MASKS, 3), torch.float32)
        rep, ok8 = guarded((B, 6), torch.int32)
        eng.gms_assign(d_votes, d_fg, Zc, lab, N_MASKS, info, min_pixels, ids=ids, masks=masks, centers=cen, report=rep)
        for b in rows:
            r = want[b]
            np.testing.assert_array_equal(ids[b].cpu().numpy(), r["raw_ids"])
            c = int(r["report"][0])
            np.testing.assert_array_equal(masks[b].cpu().numpy(), np.stack([(r["raw_ids"] == k + 1) * np.uint8(255) for k in range(N_MASKS)]))
            assert np.array_equal(cen[b, :c].cpu().numpy().view(np.uint32), r["centers"].view(np.uint32)) and not cen[b, c:].any()
            assert rep[b].tolist() == r["report"].tolist()
        assert ok5() and ok6() and ok7() and ok8()
    assert ok1() and ok2() and ok3() and ok4()


def test_truncation_and_every_cluster_too_small():
    h, w = 37, 53
    votes, fg, first, draws, want = batch(h, w)
    eng = _engine(h, w)
    r = want[0]
    Zc, lab = dev(r["seeds"][None]), dev(r["seed_labels"][None])
    P, _ = compact_np(votes[0], fg[0], 5)
    _, l = assign_np(P, r["seeds"], r["seed_labels"])
    for min_pixels, n_masks in ((20, 2), (10 ** 5, 4), (0, 3)):
        got = eng.gms_assign(dev(votes[:1]), dev(fg[:1]), Zc, lab, n_masks, None, min_pixels)
        pid, cen, rep = filter_np(l, r["seeds"], r["seed_labels"], min_pixels, n_masks)
        raw = np.zeros(h * w, np.int32)
        raw[fg[0].reshape(-1) != 0] = pid
        np.testing.assert_array_equal(got["ids"][0].cpu().numpy(), raw.reshape(h, w))
        assert got["report"][0].tolist() == rep.tolist() + [0, len(P)]
        assert np.array_equal(got["centers"][0, :len(cen)].cpu().numpy().view(np.uint32), cen.view(np.uint32))
    assert filter_np(l, r["seeds"], r["seed_labels"], 20, 2)[2][3] == 1 and filter_np(l, r["seeds"], r["seed_labels"], 10 ** 5, 4)[2][0] == 0


def test_link_reaches_the_mode_branch():
    from test_gms_cpu import chain_cases
    eng = _engine(24, 32)
    cases = list(chain_cases().values())
    got = eng.gms_link(dev(np.stack([Z for Z, _ in cases])), None, 0.05).cpu().numpy()
    assert got.tolist() == [want for _, want in cases]


def test_far_seed_keeps_its_position_and_identical_votes_make_one_cluster():
    h, w = 24, 32
    votes, fg, first, draws, want = batch(h, w)
    eng = _engine(h, w)
    Z0 = np.zeros((B, 2, 3), np.float32)
    Z0[:, 0] = 100.0
    Z0[:, 1] = compact_np(votes[0], fg[0], 5)[1][4]
    Z = eng.gms_climb(dev(votes), dev(fg), seeds=dev(Z0), sigma=0.02, iters=10).cpu().numpy()
    assert np.array_equal(Z[:, 0], Z0[:, 0]) and not np.array_equal(Z[0, 1], Z0[0, 1]) and np.array_equal(Z[1], Z0[1])      # frame 1 has no points
    flat = votes.copy()
    flat[:] = flat[:, :, 5:6, 5:6]
    g = small_options()
    out = eng.gms(dev(flat), dev(fg), dev(first), dev(draws.view(np.int32)), g, N_MASKS)
    for b in (0, 2):
        r = gms_np(flat[b], fg[b], first[b], draws[b], g, N_MASKS)
        assert r["indices"][1:].tolist() == [0] * (len(r["indices"]) - 1)                 # total == 0
        np.testing.assert_array_equal(out["indices"][b, :len(r["indices"])].cpu().numpy(), r["indices"])
        np.testing.assert_array_equal(out["ids"][b].cpu().numpy(), r["ids"])
        assert out["report"][b].tolist() == r["report"].tolist() and r["report"][1] == 1


@pytest.mark.parametrize("h,w", SHAPES)
def test_imp_equals_contract(h, w):
    k = 6
    maps = np.stack([voronoi_map(h, w, k, seed=h + b) for b in range(B)])
    maps[1][maps[1] == 2] = 0                                # an absent id
    maps[2, :3, :3] = 77                                     # outside 0..n_ids: counts as 0
    eng = _engine(h, w)
    for imp in (IMP(9, True), IMP(3, False), IMP(15, True)):
        ids, ok1 = guarded((B, h, w), torch.int32)
        ids.copy_(dev(maps))
        masks, ok2 = guarded((B, k, h, w), torch.uint8, shift=16)
        cen = dev(np.arange(B * k * 3, dtype=np.float32).reshape(B, k, 3) + 1)
        rep, ok3 = guarded((B, 6), torch.int32)
        rep.fill_(-7)
        out = eng.gms_imp(ids, k, imp, k, masks=masks, centers=cen, report=rep)
        for b in range(B):
            want, wrep, keep = imp_np(maps[b], k, imp.ksize, imp.largest)
            np.testing.assert_array_equal(out["ids"][b].cpu().numpy(), want, err_msg="%r frame %d" % (imp, b))
            np.testing.assert_array_equal(masks[b].cpu().numpy(), np.stack([(want == i + 1) * np.uint8(255) for i in range(k)]))
            assert rep[b].tolist() == [wrep[0], -7, -7, -7, wrep[1], -7]
            c = cen[b].cpu().numpy()
            assert np.array_equal(c[:len(keep)], (np.arange(k * 3, dtype=np.float32).reshape(k, 3) + 1 + b * k * 3)[[o - 1 for o in keep]])
            assert not c[len(keep):].any()
        assert ok1() and ok2() and ok3()
    assert (imp_np(maps[0], k, 9, True)[0] != maps[0]).sum() > 0.1 * h * w       # the maps exercise it


@pytest.mark.parametrize("h,w", SHAPES)
def test_chain_equals_contract_and_is_reproducible(h, w):
    votes, fg, first, draws, _ = batch(h, w)
    g = small_options(imp=IMP(5, True), min_pixels=5)
    want = [gms_np(votes[b], fg[b], first[b], draws[b], g, N_MASKS) for b in range(B)]
    for b in range(B):
        assert decidable(compact_np(votes[b], fg[b], g.subsample)[0], want[b]["seeds"], want[b]["seed_labels"], g.epsilon)
    eng = _engine(h, w)
    args = lambda v, f, fi, dr: (dev(v), dev(f), dev(fi), dev(dr.view(np.int32)))
    shapes = {"indices": ((B, 40), torch.int32), "seeds": ((B, 40, 3), torch.float32), "seed_labels": ((B, 40), torch.int32),
              "info": ((B, 3), torch.int32), "raw_ids": ((B, h, w), torch.int32), "ids": ((B, h, w), torch.int32),
              "masks": ((B, N_MASKS, h, w), torch.uint8), "centers": ((B, N_MASKS, 3), torch.float32), "report": ((B, 6), torch.int32)}
    bufs = {k: guarded(s, d) for k, (s, d) in shapes.items()}
    out = {k: v[0] for k, v in bufs.items()}

    def check(o, rows, frames):
        for b, r in zip(rows, frames):
            s, c = len(r["indices"]), int(r["report"][0])
            np.testing.assert_array_equal(o["indices"][b].cpu().numpy(), np.concatenate([r["indices"], -np.ones(40 - s, np.int32)]))
            np.testing.assert_array_equal(o["seed_labels"][b].cpu().numpy(), np.concatenate([r["seed_labels"], -np.ones(40 - s, np.int32)]))
            assert o["info"][b].tolist() == r["info"].tolist() and o["report"][b].tolist() == r["report"].tolist()
            np.testing.assert_array_equal(o["raw_ids"][b].cpu().numpy(), r["raw_ids"])
            np.testing.assert_array_equal(o["ids"][b].cpu().numpy(), r["ids"])
            np.testing.assert_array_equal(o["masks"][b].cpu().numpy(), np.stack([(r["ids"] == k + 1) * np.uint8(255) for k in range(N_MASKS)]))
            assert s == 0 or np.abs(o["seeds"][b, :s].cpu().numpy() - r["seeds"]).max() < 1e-5
            assert np.abs(o["centers"][b, :c].cpu().numpy() - r["centers"]).max(initial=0) < 1e-5 and not o["centers"][b, c:].any()

    eng.gms(*args(votes, fg, first, draws), g, N_MASKS, out=out)
    check(out, range(B), want)
    bits = {k: v.clone() for k, v in out.items()}
    # other inputs into the same tensors: every output is overwritten (frame 0 now has no foreground, frame 1 has)
    votes2, fg2, first2, draws2, _ = batch(h, w, seed=1)
    perm = [1, 0, 2]
    want2 = [gms_np(votes2[p], fg2[p], first2[p], draws2[p], g, N_MASKS) for p in perm]
    eng.gms(*args(votes2[perm], fg2[perm], first2[perm], draws2[perm]), g, N_MASKS, out=out)
    check(out, range(B), want2)
    # the first inputs again: equal bits; a frame alone equals the frame in its batch
    eng.gms(*args(votes, fg, first, draws), g, N_MASKS, out=out)
    for k in out:
        assert torch.equal(out[k].view(torch.uint8), bits[k].view(torch.uint8)), k
    alone = eng.gms(*args(votes[:1], fg[:1], first[:1], draws[:1]), g, N_MASKS)
    for k in out:
        assert torch.equal(alone[k][0].view(torch.uint8), bits[k][0].view(torch.uint8)), k
    assert all(ok() for _, ok in bufs.values())


def test_full_frame_480x640():
    """All pixels foreground: the largest n_sub (61 440), the reference's 200 seeds, the real plane size of the IMP."""
    h, w, k = 480, 640, 5
    rng = np.random.RandomState(3)
    centres = np.array([[0.25 * j - 0.5, 0.1 * (j % 2) - 0.05, 0.8 + 0.05 * j] for j in range(k)])
    yy, xx = np.mgrid[:h, :w]
    which = np.clip(((xx + 12 * np.sin(yy / 17.0)) * k / w).astype(int), 0, k - 1)
    salt = rng.rand(h, w) < 0.01
    which[salt] = rng.randint(0, k, int(salt.sum()))
    votes = np.ascontiguousarray((centres[which].transpose(2, 0, 1) + 0.003 * rng.randn(3, h, w)).astype(np.float32))
    fg = np.ones((h, w), np.uint8)
    g = GaussianMeanShift()
    first, draws = GaussianMeanShift(seed=11).draws([g.n_sub(h * w)])
    want = gms_np(votes, fg, first[0], draws[0], g, 16)
    assert want["info"].tolist() == [h * w, 61440, 200] and want["report"][0] == k
    assert decidable(compact_np(votes, fg, 5)[0], want["seeds"], want["seed_labels"], g.epsilon)
    assert (want["ids"] != want["raw_ids"]).sum() > 1000                                   # the IMP removes the salt
    out = _engine(h, w, batch=1).gms(dev(votes[None]), dev(fg[None]), dev(first), dev(draws.view(np.int32)), g, 16)
    np.testing.assert_array_equal(out["indices"][0].cpu().numpy(), want["indices"])
    np.testing.assert_array_equal(out["seed_labels"][0].cpu().numpy(), want["seed_labels"])
    np.testing.assert_array_equal(out["raw_ids"][0].cpu().numpy(), want["raw_ids"])
    np.testing.assert_array_equal(out["ids"][0].cpu().numpy(), want["ids"])
    assert out["report"][0].tolist() == want["report"].tolist()
    np.testing.assert_array_equal(out["masks"][0, :k].cpu().numpy(), np.stack([(want["ids"] == i + 1) * np.uint8(255) for i in range(k)]))


@pytest.mark.parametrize("name", FIXTURES)
def test_chain_on_the_reference_fixtures(name):
    g = np.load(os.path.join(GOLDEN, name))
    opt = fixture_options(g)
    h, w = g["fg"].shape
    out = _engine(h, w).gms(dev(g["votes"][None]), dev(g["fg"][None]), dev(g["first"].reshape(1)), dev(g["draws"].view(np.int32)[None]), opt, N_MASKS)
    np.testing.assert_array_equal(out["indices"][0].cpu().numpy(), g["indices"])
    np.testing.assert_array_equal(out["seed_labels"][0].cpu().numpy(), g["seed_labels"])
    np.testing.assert_array_equal(out["ids"][0].cpu().numpy(), g["clustered"])                         # (a): labels exactly
    assert same_partition(out["ids"][0].cpu().numpy(), g["clustered_multinomial"])                    # (b): as partitions
    assert np.abs(out["seeds"][0].cpu().numpy() - g["seeds"]).max() < 1e-5
    assert np.abs(out["centers"][0, :len(g["centers"])].cpu().numpy() - g["centers"]).max() < 1e-5


def test_bad_arguments_are_refused():
    h, w = 24, 32
    votes, fg, first, draws, _ = batch(h, w)
    eng = _engine(h, w)
    a = (dev(votes), dev(fg), dev(first), dev(draws.view(np.int32)))
    for bad in (dict(subsample=0), dict(subsample=65)):
        with pytest.raises(engine._lib.QuberError):
            eng.gms_seeds(*a, **bad)
    with pytest.raises(engine._lib.QuberError):
        eng.gms_climb(a[0], a[1], seeds=dev(np.zeros((B, 4, 3), np.float32)), sigma=0.0)
    with pytest.raises(engine._lib.QuberError):
        eng.gms_link(dev(np.zeros((B, 4, 3), np.float32)), None, -1.0)
    with pytest.raises(engine._lib.QuberError):
        eng.gms_imp(dev(np.zeros((B, h, w), np.int32)), 255)
    big = engine.Engine(engine.make_config(1024, 1280, max_batch=1, max_instances=8, with_network=False), "cuda:0")
    try:
        with pytest.raises(ValueError):                      # 2 * 1024 * 40 * 4 bytes of planes: more than the LDS
            big.gms_imp(torch.zeros((1, 1024, 1280), dtype=torch.int32, device="cuda"), 4)
        with pytest.raises(ValueError):
            big.gms(torch.zeros((1, 3, 1024, 1280), device="cuda"), torch.zeros((1, 1024, 1280), dtype=torch.uint8, device="cuda"),
                    torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros((1, 200), dtype=torch.int32, device="cuda"))
        t = torch.zeros((1, 1024, 1280), dtype=torch.int32, device="cuda")
        assert big.lib.quber_gms_imp(big.h, engine._ptr(t), 1, 4, 9, 1, 0, None, None, None, engine._stream()) != 0      # the error code
    finally:
        big.close()


GMS_KEYS = {"cluster_masks", "cluster_ids", "cluster_raw_ids", "cluster_seeds", "cluster_centers", "cluster_report"}


def test_predictor_cluster_equals_none_fed_with_the_cluster_masks():
    """predict(..., center_votes=, fg=) under cluster=GaussianMeanShift(...) returns what a predictor without cluster= returns when it is
    given cluster_masks as its initial masks, in every key; the clustering's own keys equal the contract."""
    from quber_amd import synth
    from test_gpu_cleanup import speck_logits
    from test_gpu_masknms import _equal, _predictor
    h, w = 96, 128
    logits = speck_logits(h, w)
    sc = [synth.make_scene(3 + b, h, w, 2) for b in range(2)]
    rgb, dep = np.stack([s["rgb"] for s in sc]), np.stack([s["depth"] for s in sc])
    made = [vote_scene(h, w, 3, 41, stray=2), vote_scene(h, w, 4, 42, stray=2)]
    votes, fg = [m[0] for m in made], [m[1] for m in made]
    g = GaussianMeanShift(num_seeds=40, min_pixels=200, imp=IMP(5, True), seed=5)
    kw = dict(decode_errors=True, track_initial=True)
    twin = GaussianMeanShift(num_seeds=40, seed=5)
    draws = [twin.draws([g.n_sub(int(fg[b].sum())) for b in (0, 1)]), twin.draws([g.n_sub(int(fg[1].sum()))])]
    want = [gms_np(votes[b], fg[b], draws[0][0][b], draws[0][1][b], g, 40) for b in (0, 1)]
    want.append(gms_np(votes[1], fg[1], draws[1][0][0], draws[1][1][0], g, 40))
    for b, r in enumerate(want):
        assert decidable(compact_np(votes[min(b, 1)], fg[min(b, 1)], 5)[0], r["seeds"], r["seed_labels"], g.epsilon)
    assert [int(r["report"][0]) for r in want] == [3, 4, 4]
    got_off, want_off = [], []
    with_cluster = _predictor(h, w, logits, got_off, cluster=g, **kw)
    none = _predictor(h, w, logits, want_off, **kw)

    def check(a, b, f, what):
        assert set(a) - GMS_KEYS == set(b) and GMS_KEYS <= set(a) and not GMS_KEYS & set(b), (what, sorted(a), sorted(b))
        for key in b:
            _equal(a[key], b[key], "%s frame %d: %s" % (what, f, key))
        r = want[f]
        c = int(r["report"][0])
        np.testing.assert_array_equal(a["cluster_masks"].cpu().numpy(), np.stack([(r["ids"] == k + 1) * np.uint8(255) for k in range(c)]))
        np.testing.assert_array_equal(a["cluster_ids"].cpu().numpy(), r["ids"])
        np.testing.assert_array_equal(a["cluster_raw_ids"].cpu().numpy(), r["raw_ids"])
        assert a["cluster_report"].dtype == torch.int64 and a["cluster_report"].tolist() == r["report"].tolist()
        assert a["cluster_seeds"].shape == (40, 3) and np.abs(a["cluster_seeds"].cpu().numpy() - r["seeds"]).max() < 1e-5
        assert a["cluster_centers"].shape == (c, 3) and np.abs(a["cluster_centers"].cpu().numpy() - r["centers"]).max() < 1e-5

    outs = with_cluster.predict_batch(rgb, dep, None, center_votes=votes, fg=fg)
    refs = none.predict_batch(rgb, dep, [o["cluster_masks"].cpu().numpy() for o in outs])
    for f, (a, b) in enumerate(zip(outs, refs)):
        check(a, b, f, "predict_batch")
        assert "instances" in a
    a = with_cluster.predict(rgb[1], dep[1], center_votes=votes[1], fg=fg[1] != 0)[0]      # one frame, a bool foreground: the third frame's draws
    b = none.predict(rgb[1], dep[1], a["cluster_masks"].cpu().numpy())[0]
    check(a, b, 2, "predict")
    _equal(a["instances"], b["instances"], "instances")
    assert len(got_off) == len(want_off) >= 2
    for x, y in zip(got_off, want_off):
        assert x.shape == y.shape and torch.equal(x, y)
    from quber_amd.meanshift import MeanShift
    nan = votes[0].copy()
    nan[0, 0, 0] = np.nan
    for call in (lambda: with_cluster.predict_batch(rgb, dep, [m[:1] for m in fg], center_votes=votes, fg=fg),       # masks and votes
                 lambda: with_cluster.predict_batch(rgb, dep, None),                                               # no votes
                 lambda: with_cluster.predict_batch(rgb, dep, None, center_votes=votes),                           # no foreground
                 lambda: with_cluster.predict(rgb[0], dep[0], fg[:1]),
                 lambda: with_cluster.predict(rgb[0], dep[0], mask_scores=np.ones(2, np.float32), center_votes=votes[0], fg=fg[0]),
                 lambda: with_cluster.predict(rgb[0], dep[0], embeddings=np.zeros((64, h, w), np.float32)),        # the other clusterer's input
                 lambda: with_cluster.predict(rgb[0], dep[0], center_votes=nan, fg=fg[0]),                         # not finite
                 lambda: with_cluster.predict(rgb[0], dep[0], center_votes=votes[0][:2], fg=fg[0]),
                 lambda: none.predict_batch(rgb, dep, None, center_votes=votes, fg=fg),                            # votes without cluster=
                 lambda: with_cluster.model.predict_one(rgb[0], dep[0], np.zeros((1, h, w), np.uint8)),
                 lambda: with_cluster.model.enqueue_batch(dev(rgb), dev(dep), dev(np.zeros((2, 1, h, w), np.uint8)))):
        with pytest.raises(ValueError):
            call()
    ucn = _predictor(h, w, logits, [], cluster=MeanShift(num_seeds=8))
    with pytest.raises(ValueError):
        ucn.predict(rgb[0], dep[0], center_votes=votes[0], fg=fg[0])
    # a refused call has drawn nothing: the next frame takes the draws a fresh stream would give after three frames
    nxt = GaussianMeanShift(num_seeds=40, seed=5)
    nxt.draws([g.n_sub(int(fg[b].sum())) for b in (0, 1, 1)])
    assert g.draws([50])[1].tolist() == nxt.draws([50])[1].tolist()
    for p in (with_cluster, none, ucn):
        p.model.close()
