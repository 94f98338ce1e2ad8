"""GPU: the scene-level perturbation on the device (csrc/scene.hip through Engine.scene_perturb and MaskRefinerPredictor(scene=...))
against its numpy contract (tests/test_scene_cpu.py: scene_perturb_np).  Integers, bits and two float64 expressions: every comparison
is exact."""
import numpy as np
import pytest
import torch

from quber_amd import _lib, engine
from quber_amd.eval import coco_ap
from quber_amd.maskrefiner.predictor import MaskRefinerPredictor
from quber_amd.perturb import Perturb
from quber_amd.scene import ScenePerturb, scene_draws
from test_perturb_cpu import perturb_batch_np
from test_scene_cpu import ACT, GPU_COUNTS, GPU_FRAMES, MIN_RATIO, gpu_batch, hand_cases, random_scene, scene_perturb_np

pytestmark = pytest.mark.gpu

FILL = 0x3C
TABLES = ("fp_act", "gs_act", "merge_act", "split_act", "split_try", "delete_act")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_ENGINES = {}


def _engine(h, w, batch=3, cap=64):
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


def _guarded(shape, dtype, shift):
    """A tensor of `shape`, `shift` elements into a buffer filled with a sentinel byte -> (the whole buffer as bytes, the view)."""
    n, es = int(np.prod(shape)), torch.empty((), dtype=dtype).element_size()
    raw = torch.full(((shift + n + 64) * es,), FILL, dtype=torch.uint8, device="cuda")
    return raw, raw.view(dtype)[shift:shift + n].view(shape)


def _intact(raw, view, shift):
    es, n = view.element_size(), view.numel()
    return bool((raw[:shift * es] == FILL).all()) and bool((raw[(shift + n) * es:] == FILL).all())


class Outputs:
    def __init__(self, B, M, h, w, shift):
        self.shift = shift
        self.bufs = {"out": _guarded((B, M, h, w), torch.uint8, shift), "info": _guarded((B, M, 4), torch.int32, shift),
                     "report": _guarded((B, 8), torch.int32, shift)}

    def intact(self):
        return all(_intact(raw, view, self.shift) for raw, view in self.bufs.values())


def _run(eng, gt, props, n_gt, n_prop, draws, M, ratio, shift=16, outs=None, garbage=True):
    """Engine.scene_perturb into guarded outputs, the inputs `shift` bytes into sentinel-filled allocations, the rows behind the frames'
    counts filled with garbage on the device -> (masks, info, report) on the host."""
    B, N, h, w = gt.shape
    rng = np.random.RandomState(5)
    g_in, p_in = gt.copy(), props.copy()
    act = {k: np.array(draws[k]) for k in TABLES}
    if garbage:
        for b in range(B):
            g_in[b, n_gt[b]:] = rng.randint(0, 256, g_in[b, n_gt[b]:].shape)
            p_in[b, n_prop[b]:] = rng.randint(0, 256, p_in[b, n_prop[b]:].shape)
            act["fp_act"][b, n_prop[b]:] = 1                 # a coin of a proposal that is not there
            act["gs_act"][b, n_prop[b]:] = 1
    raws = [_guarded(a.shape, torch.uint8, shift) for a in (g_in, p_in)]
    for (raw, view), a in zip(raws, (g_in, p_in)):
        view.copy_(dev(a))
    o = Outputs(B, M, h, w, shift) if outs is None else outs
    v = {k: b[1] for k, b in o.bufs.items()}
    r = eng.scene_perturb(raws[0][1], raws[1][1], dev(n_gt.astype(np.int32)), dev(n_prop.astype(np.int32)), {k: dev(a) for k, a in act.items()},
                          M, ratio, v["out"], v["info"], v["report"])
    assert r["masks"].data_ptr() == v["out"].data_ptr()
    torch.cuda.synchronize()
    assert o.intact(), "wrote outside an output"
    for (raw, view), a in zip(raws, (g_in, p_in)):
        assert _intact(raw, view, shift)
        np.testing.assert_array_equal(view.cpu().numpy(), a, err_msg="an input changed")
    return tuple(v[k].cpu().numpy() for k in ("out", "info", "report"))


def _same(got, want, what=""):
    for name, a, b in zip(("report", "info", "masks"), got[::-1], want[::-1]):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg="%s %s" % (what, name))


@pytest.mark.parametrize("N,P,M", GPU_COUNTS, ids=["N%d-P%d-M%d" % c for c in GPU_COUNTS])
@pytest.mark.parametrize("h,w", GPU_FRAMES, ids=["%dx%d" % s for s in GPU_FRAMES])
def test_scene_perturb_equals_contract(h, w, N, P, M):
    """Batch 3 with different n_gt / n_prop per frame; (24, 40) one word plus tail, (33, 64) whole words and the 16-byte paths,
    (37, 70) tail bits, (20, 131) five words per row: the horizontal dilation carries across words in both directions."""
    s = gpu_batch((h, w), N, P, M)
    assert not s["want"][2][:, 7].any()                      # chosen on the CPU: the contract alone drops nothing
    eng = _engine(h, w)
    for shift in (16, 3):                                    # 16 bytes into the allocations (the 16-byte paths where W allows) and 3 (the byte paths)
        got = _run(eng, s["gt"], s["props"], s["n_gt"], s["n_prop"], s["draws"], M, s["ratio"], shift)
        _same(got, s["want"], "%dx%d N=%d P=%d M=%d shift %d" % (h, w, N, P, M, shift))


def test_frame_with_more_rows_and_columns_than_a_workgroup_has_lanes():
    """264 x 528: the row / column counts of an entry and their prefix sums take more than one element per lane (the kernels' workgroups
    have 256), a plane more than one block of the per-word kernels."""
    h, w = 264, 528
    s = gpu_batch((h, w), 5, 5, 16)
    assert s["want"][2][:, 5].sum() > 0 and s["want"][2][:, 4].sum() > 0          # splits and merges happen
    for shift in (16, 3):
        got = _run(_engine(h, w), s["gt"], s["props"], s["n_gt"], s["n_prop"], s["draws"], 16, s["ratio"], shift)
        _same(got, s["want"], "264x528 shift %d" % shift)


def test_hand_drawn_cases_on_the_device():
    cases = hand_cases()
    assert len(cases) > 30
    dropped = 0
    for i, (gt, props, M, d, ratio) in enumerate(cases):
        h, w = gt.shape[1:]
        want = scene_perturb_np(gt, props, len(gt), len(props), M, ratio, d)
        dropped += int(want[2][7] > 0)
        n_gt, n_prop = np.array([len(gt)], np.int32), np.array([len(props)], np.int32)
        got = _run(_engine(h, w), gt[None], props[None], n_gt, n_prop, {k: d[k][None] for k in TABLES}, M, ratio, shift=1, garbage=False)
        _same(got, tuple(a[None] for a in want), "hand case %d" % i)
    assert dropped == 2                                      # capacity reached in step 3 and in step 5: the only cases that drop


def test_seeded_scenes_of_the_cpu_test_on_the_device():
    """The scenes of test_contract_equals_the_reference_description_on_random_scenes (frames of 20-50 x 20-70, each its own size)."""
    tot = np.zeros(8, np.int64)
    for seed in range(24):
        s = random_scene(seed)
        gt, props = s["gt"], s["props"]
        want = scene_perturb_np(gt, props, len(gt), len(props), s["M"], MIN_RATIO, s["d"])
        assert want[2][7] == 0
        tot += want[2]
        h, w = gt.shape[1:]
        got = _run(_engine(h, w), gt[None], props[None], np.array([len(gt)], np.int32), np.array([len(props)], np.int32),
                   {k: s["d"][k][None] for k in TABLES}, s["M"], MIN_RATIO, shift=16 if seed % 2 else 5, garbage=False)
        _same(got, tuple(a[None] for a in want), "seed %d" % seed)
    assert (tot[:7] > 0).all(), tot


def test_second_call_overwrites():
    h, w = 33, 64
    eng = _engine(h, w)
    a, b = gpu_batch((h, w), 17, 17, 40), gpu_batch((h, w), 1, 5, 40, ratio=0.9)
    assert b["want"][2][:, 0].max() < a["want"][2][:, 0].min() and b["want"][1].any()      # far fewer masks than the first call left behind
    o = Outputs(3, 40, h, w, 16)
    _same(_run(eng, a["gt"], a["props"], a["n_gt"], a["n_prop"], a["draws"], 40, a["ratio"], 16, o), a["want"])
    _same(_run(eng, b["gt"], b["props"], b["n_gt"], b["n_prop"], b["draws"], 40, b["ratio"], 16, o), b["want"], "second call")


def test_bad_arguments_are_refused_and_launch_nothing():
    h, w = 24, 40
    eng = _engine(h, w, cap=8)
    s = gpu_batch((h, w), 5, 5, 16)
    gt, props, n_gt, n_prop = dev(s["gt"]), dev(s["props"]), dev(s["n_gt"]), dev(s["n_prop"])
    d = {k: dev(s["draws"][k]) for k in TABLES}
    o = Outputs(3, 16, h, w, 4)
    v = {k: b[1] for k, b in o.bufs.items()}
    P = engine._ptr
    good = [P(gt), P(props), P(n_gt), P(n_prop), 3, 5, 5, 16, 0.05, P(d["fp_act"]), P(d["gs_act"]), P(d["merge_act"]), P(d["split_act"]),
            P(d["split_try"]), P(d["delete_act"]), P(v["out"]), P(v["info"]), P(v["report"])]
    call = lambda a: eng.lib.quber_scene_perturb(eng.h, *a, engine._stream())
    change = lambda i, x: [x if j == i else y for j, y in enumerate(good)]
    before = eng.lib.quber_workspace_bytes(eng.h)
    assert call(change(4, 4)) != 0                                                      # above max_batch
    assert call(change(5, 252)) != 0 and b"256" in eng.lib.quber_last_error()          # N + P = 257: an error, not a clamp
    assert call(change(6, 252)) != 0
    assert call(change(5, -1)) != 0 and call(change(6, -1)) != 0
    assert call(change(7, 257)) != 0 and b"max_masks" in eng.lib.quber_last_error()
    assert call(change(7, 0)) != 0
    assert call(change(8, -0.5)) != 0 and call(change(8, float("nan"))) != 0
    for i in (0, 1, 2, 3, 9, 10, 11, 12, 13, 14, 15, 16, 17):
        assert call(change(i, None)) != 0 and b"null" in eng.lib.quber_last_error(), i
    torch.cuda.synchronize()
    assert o.intact() and all(bool((x.view(torch.uint8) == FILL).all()) for x in v.values()), "a refused call wrote"
    assert eng.lib.quber_workspace_bytes(eng.h) == before, "a refused call allocated"
    # the row counts are not bounded by max_instances (8 here); the first good call allocates the workspace, which
    # quber_workspace_bytes then counts; an equal call allocates nothing
    assert call(good) == 0
    b1 = eng.lib.quber_workspace_bytes(eng.h)
    assert call(good) == 0
    torch.cuda.synchronize()
    assert b1 > before and eng.lib.quber_workspace_bytes(eng.h) == b1
    _same(tuple(v[k].cpu().numpy() for k in ("out", "info", "report")), s["want"])


# ---- the workspaces that grow on demand ----
GROW_FRAME = (33, 65)                   # rows that are not whole words, planes padded to 4 words, a pixel count that is no multiple of 16


def _scene_call(B, N, P, M, seed):
    """-> the arguments of _run behind the engine: B frames of N ground truths and P proposals at GROW_FRAME, tables at capacity M."""
    h, w = GROW_FRAME
    gt, props, per = np.zeros((B, N, h, w), np.uint8), np.zeros((B, P, h, w), np.uint8), []
    for b in range(B):
        sc = random_scene(seed + b, GROW_FRAME, N, P)
        gt[b], props[b] = sc["gt"], sc["props"]
        per.append(scene_draws(np.random.RandomState(seed + b + 7), P, M, h, w, *ACT))
    draws = {k: np.ascontiguousarray(np.stack([d[k] for d in per])) for k in TABLES}
    return gt, props, np.full(B, N, np.int32), np.full(B, P, np.int32), draws, M, MIN_RATIO


def _coco_call(B, n_dt, n_gt, seed):
    """-> dt u8 [B,n_dt,h,w], scores f32 [B,n_dt], gt u8 [B,n_gt,h,w]: rectangles, the first detections shifted ground truths."""
    h, w = GROW_FRAME
    rng = np.random.RandomState(seed)

    def rects(n):
        m = np.zeros((B, n, h, w), np.uint8)
        for plane in m.reshape(-1, h, w):
            y, x = rng.randint(0, h - 8), rng.randint(0, w - 8)
            plane[y:y + rng.randint(4, h - y), x:x + rng.randint(4, w - x)] = 1
        return m

    gt, dt = rects(n_gt), rects(n_dt)
    k = min(n_dt, n_gt)
    dt[:, :k] = np.roll(gt[:, :k], 2, 3)
    return dt, rng.random_sample((B, n_dt)).astype(np.float32), gt


def _coco_run(eng, dt, scores, gt):
    """quber_coco_match (segm, every ground truth present, computed areas) -> its ten outputs on the host."""
    B, n_dt, n_gt = dt.shape[0], dt.shape[1], gt.shape[1]
    T, A, TOP = len(coco_ap.IOU_THRS), len(coco_ap.AREA_RNG), coco_ap.TOP
    outs = [torch.full(shape, FILL, dtype=dtype, device="cuda") for dtype, shape in (
        (torch.int32, (B, 2)), (torch.int32, (B, TOP)), (torch.float32, (B, TOP)), (torch.float64, (B, TOP)), (torch.float64, (B, n_gt)),
        (torch.float64, (B, TOP, n_gt)), (torch.uint8, (B, A, T, TOP)), (torch.uint8, (B, A, T, TOP)), (torch.uint8, (B, A, n_gt)),
        (torch.int32, (B, A, n_gt)))]
    ins = [dev(dt), dev(scores), dev(gt), torch.zeros((B, n_gt), dtype=torch.uint8, device="cuda"), dev(coco_ap.IOU_THRS), dev(coco_ap.AREA_RNG)]
    P = engine._ptr
    _lib.check(eng.lib.quber_coco_match(eng.h, P(ins[0]), P(ins[1]), None, n_dt, P(ins[2]), P(ins[3]), None, None, n_gt, B, 0, P(ins[4]), T, P(ins[5]), A,
                                        *[P(o) for o in outs], engine._stream()))
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def _bitwise(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, i)


def test_growing_workspaces_of_scene_perturb_and_coco_match():
    """The two entries whose workspace grows with the call (the third, quber_perturb_masks, has its own test in test_gpu_perturb.py), on
    an engine of max_batch 2: a small call, a larger one, the small one again.  The third result equals the first bit for bit - the
    small layout inside the larger buffer; quber_workspace_bytes rises by the layout total of the first call, then to the total of the
    larger one, and stays; an engine that has only ever seen the larger call computes the same."""
    h, w = GROW_FRAME
    make = lambda: engine.Engine(engine.make_config(h, w, max_batch=2, max_instances=64, with_network=False), "cuda:0")
    ws = lambda e, which, b, n, m: int(e.lib.quber_debug_ws_bytes(which, b, n, m, h, w, 0))
    small_s, large_s = _scene_call(1, 2, 1, 4, 500), _scene_call(2, 5, 4, 16, 600)
    small_c, large_c = _coco_call(1, 3, 2, 700), _coco_call(2, 9, 17, 800)
    eng, fresh = make(), make()
    try:
        for what, run, small, large, need_small, need_large in (
                ("scene", lambda e, a: _run(e, *a), small_s, large_s, ws(eng, 2, 1, 3, 4), ws(eng, 2, 2, 9, 16)),
                ("coco", lambda e, a: _coco_run(e, *a), small_c, large_c, ws(eng, 1, 1, 2, 0), ws(eng, 1, 2, 17, 0))):
            assert 0 < need_small < need_large, what
            b0 = eng.workspace_bytes()
            first = run(eng, small)
            assert eng.workspace_bytes() == b0 + need_small, what
            second = run(eng, large)
            assert eng.workspace_bytes() == b0 + need_large, what       # the small buffer was freed, not kept beside the new one
            third = run(eng, small)
            assert eng.workspace_bytes() == b0 + need_large, what       # never shrinks, allocates nothing
            _bitwise(third, first, what + ": the small call after the larger one")
            f0 = fresh.workspace_bytes()
            _bitwise(run(fresh, large), second, what + ": a fresh engine on the larger call")
            assert fresh.workspace_bytes() == f0 + need_large, what
            assert any(a.any() for a in first[:1]) and any(a.any() for a in second[:1]), what      # the calls did something
    finally:
        eng.close()
        fresh.close()


# ---- end to end ----
def _equal(a, b, path):
    """Bit for bit, through tensors, tuples, dicts and Instances."""
    if isinstance(b, torch.Tensor):
        assert isinstance(a, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
    elif isinstance(b, dict):
        assert set(a) == set(b), path
        for k in b:
            _equal(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(b, (tuple, list)):
        assert len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, "%s[%d]" % (path, k))
    elif hasattr(b, "get_fields"):
        fa, fb = a.get_fields(), b.get_fields()
        assert set(fa) == set(fb), path
        for k in fb:
            _equal(fa[k].tensor if hasattr(fa[k], "tensor") else fa[k], fb[k].tensor if hasattr(fb[k], "tensor") else fb[k], path + "." + k)
    else:
        assert a == b, path


SCENE_KEYS = {"scene_masks", "scene_info", "scene_report"}


def test_predictor_scene_equals_none_fed_with_the_contract():
    """MaskRefinerPredictor(scene=ScenePerturb(...)) on ground truth and proposals = the same predictor without scene fed the contract's
    masks, in every output key (random weights, 64 x 96: the network runs); chained into perturb= with the scene's walk targets, the
    perturbed masks are perturb_batch_np of the contract's output."""
    from quber_amd import synth
    h, w, B, M = 64, 96, 2, 12
    sc = [synth.make_scene(11 + b, h, w, 2) for b in range(B)]
    rgb, dep = np.stack([s["rgb"] for s in sc]), np.stack([s["depth"] for s in sc])
    scene = ScenePerturb(seed=3, max_masks=M, min_mask_ratio=MIN_RATIO, fp=0.6, gs=0.6, merge=0.4, split=0.6, delete=0.2)
    frames = [random_scene(900 + b, (h, w), 4 - b, 3 + b) for b in range(B)]     # frame 1 has fewer ground truths and more proposals
    gts, props = [f["gt"] for f in frames], [f["props"] for f in frames]
    P = max(len(p) for p in props)
    draws = scene.draws(B, P, h, w)
    want = [scene_perturb_np(gts[b], props[b], len(gts[b]), len(props[b]), M, MIN_RATIO, {k: v[b] for k, v in draws.items()}) for b in range(B)]
    assert all(0 < r[2][0] < M and r[2][7] == 0 for r in want) and sum(int(r[2][1] + r[2][2]) for r in want) > 0
    assert any(not np.array_equal(r[0][:len(g)], g * 255) for r, g in zip(want, gts))     # the stage did something
    fed = [r[0][:r[2][0]] for r in want]
    kw = dict(decode_errors=True, track_initial=True)
    with_scene = MaskRefinerPredictor(None, device="cuda:0", scene=scene, **kw)
    sd = with_scene.model.state_dict
    none = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, **kw)

    def check(a, b, f, what):
        assert set(a) - SCENE_KEYS == set(b) and SCENE_KEYS <= set(a) and not SCENE_KEYS & set(b), (what, sorted(a), sorted(b))
        for key in b:
            _equal(a[key], b[key], "%s frame %d: %s" % (what, f, key))
        r = want[f]
        n = int(r[2][0])
        np.testing.assert_array_equal(a["scene_masks"].cpu().numpy(), r[0][:n])
        assert a["scene_info"].dtype == torch.int64 and a["scene_report"].dtype == torch.int64
        np.testing.assert_array_equal(a["scene_info"].cpu().numpy(), r[1][:n])
        np.testing.assert_array_equal(a["scene_report"].cpu().numpy(), r[2])

    outs = with_scene.predict_batch(rgb, dep, gts, proposals=props)
    refs = none.predict_batch(rgb, dep, fed)
    for f, (a, b) in enumerate(zip(outs, refs)):
        check(a, b, f, "predict_batch")
    # predict(): one frame, bool masks; frame 0 alone draws RandomState(seed + 0) with ITS number of proposal rows
    d0 = scene.draws(1, len(props[0]), h, w)
    w0 = scene_perturb_np(gts[0], props[0], len(gts[0]), len(props[0]), M, MIN_RATIO, {k: v[0] for k, v in d0.items()})
    one = with_scene.predict(rgb[0], dep[0], gts[0] != 0, proposals=props[0] != 0)[0]
    np.testing.assert_array_equal(one["scene_masks"].cpu().numpy(), w0[0][:w0[2][0]])
    np.testing.assert_array_equal(one["scene_report"].cpu().numpy(), w0[2])
    # no proposals at all: P = 0
    bare = with_scene.predict(rgb[0], dep[0], gts[0])[0]
    dz = scene.draws(1, 0, h, w)
    wz = scene_perturb_np(gts[0], props[0][:0], len(gts[0]), 0, M, MIN_RATIO, {k: v[0] for k, v in dz.items()})
    np.testing.assert_array_equal(bare["scene_masks"].cpu().numpy(), wz[0][:wz[2][0]])
    # chained into perturb=: the walk's targets are the scene's draw 8, the walk acts on the scene's output
    walk = Perturb(scene.walk_targets(B, P, h, w), seed=5, rounds=6)
    chained = MaskRefinerPredictor(None, device="cuda:0", state_dict=sd, scene=scene, perturb=walk)
    outs = chained.predict_batch(rgb, dep, gts, proposals=props)
    pm, pr = perturb_batch_np(np.stack([r[0] for r in want]), walk.programs(B, M, h, w), walk.targets(B, M))
    for f, o in enumerate(outs):
        n = int(want[f][2][0])
        np.testing.assert_array_equal(o["scene_masks"].cpu().numpy(), want[f][0][:n])
        np.testing.assert_array_equal(o["perturbed_masks"].cpu().numpy(), pm[f, :n])
        np.testing.assert_array_equal(o["perturb_report"].cpu().numpy(), pr[f, :n])
    assert not np.array_equal(pm, np.stack([r[0] for r in want]))
    # what has no scene form says so
    with pytest.raises(ValueError, match="scene"):
        with_scene.model.enqueue_batch(dev(rgb), dev(dep), dev(np.stack([r[0] for r in want])))
    with pytest.raises(ValueError, match="scene"):
        none.predict_batch(rgb, dep, gts, proposals=props)
    for p in (with_scene, none, chained):
        p.model.close()
