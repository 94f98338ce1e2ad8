"""Dilated Winograd layers with the phases of an axis packed into shared tiles (option key 51; csrc/winograd_xf.h: Axis): the
three-kernel pipeline through quber_op_conv3x3_winograd against the direct kernel, float64 and the per-phase tiling; the network
with key 51 = 1 against 0; the stage profiler's FLOPs against the tile counts written out here."""
import ctypes as C

import numpy as np
import pytest
import torch

from quber_amd import _lib, arch, engine, synth

pytestmark = pytest.mark.gpu


def ceil_div(a, b):
    return -(-a // b)


def axis_tiles(n, d, m):
    """(tiles per phase, tiles packed) of one axis: d phases of ceil(ceil(n/d)/m) tiles each, or the non-empty phases in a row
    with one zero slot between neighbours"""
    per_phase = d * ceil_div(ceil_div(n, d), m)
    packed = ceil_div(n + min(d, n) - 1, m)
    return per_phase, packed


def tiles(H, W, d, m, pack):
    ty, tx = axis_tiles(H, d, m), axis_tiles(W, d, m)
    return (min(ty) if pack else ty[0]) * (min(tx) if pack else tx[0])


CASES = [
    # B, H, W, Cin, Cout, d
    (2, 30, 40, 128, 128, 6),      # rows packed (m = 4: 12 -> 9), columns per phase
    (1, 30, 40, 128, 128, 8),      # columns packed (16 -> 12), rows per phase
    (2, 23, 37, 64, 128, 4),       # phases of unequal size
    (1, 7, 9, 64, 64, 12),         # one-pixel phases: a tile spans three or more phases
    (3, 13, 5, 32, 64, 3),         # a block of the transforms spans images
    (1, 5, 6, 32, 32, 8),          # d > H, W: empty phases
]
_REF = {}


def _inputs(case):
    """input, filters, affine and the float64 result of a case: computed once, shared by the three tile sizes"""
    if case not in _REF:
        B, H, W, Cin, Cout, d = case
        g = torch.Generator(device="cuda").manual_seed(11)
        x = torch.randn(B, H, W, Cin, device="cuda", generator=g)
        w = torch.randn(Cout, Cin, 3, 3, device="cuda", generator=g) / np.sqrt(Cin * 9)
        sc = torch.rand(Cout, device="cuda", generator=g) + 0.5
        sh = torch.randn(Cout, device="cuda", generator=g)
        ref = torch.nn.functional.conv2d(x.cpu().double().permute(0, 3, 1, 2), w.cpu().double(), padding=d, dilation=d)
        ref = (ref * sc.cpu().double()[None, :, None, None] + sh.cpu().double()[None, :, None, None]).permute(0, 2, 3, 1).contiguous()
        _REF[case] = (x, w, sc, sh, ref)
    return _REF[case]


@pytest.mark.parametrize("m", [2, 4, 6])
@pytest.mark.parametrize("case", CASES)
def test_packed_winograd_op(case, m):
    B, H, W, Cin, Cout, d = case
    relu = CASES.index(case) % 2
    tol = {2: 1e-5, 4: 2e-5, 6: 1e-4}[m]          # the bounds of test_gpu_parity.py::test_conv3x3_winograd_vs_float64
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    x, w, sc, sh, ref = _inputs(case)
    if relu:
        ref = ref.relu()
    P = (m + 2) ** 2
    u = torch.empty(P * Cout * Cin, device="cuda")
    ws = torch.empty(P * B * tiles(H, W, d, m, False) * (Cin + Cout), device="cuda")      # the per-phase bound, as the existing tests size it

    def run(pack):
        y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
        lib.quber_set_tuning(51, pack)
        _lib.check(lib.quber_op_conv3x3_winograd(p(x), B, H, W, Cin, p(w), Cout, d, m, p(sc), p(sh), relu, p(u), p(ws), ws.numel(), p(y), st))
        return y

    lib.quber_set_tuning(2, 1)
    lib.quber_set_tuning(25, 0)                   # the three-kernel pipeline
    try:
        y = run(1)
        y_again = run(1)
        y_phase = run(0)
        packed = torch.empty(Cout * 9 * Cin, device="cuda")
        yd = torch.empty_like(y)
        _lib.check(lib.quber_op_conv2d(p(x), B, H, W, Cin, p(w), Cout, 3, 1, d, d, p(sc), p(sh), p(None), relu, p(packed), p(yd), st))
        torch.cuda.synchronize()
    finally:
        lib.quber_set_tuning(51, 1)
        lib.quber_set_tuning(25, 1)
        lib.quber_set_tuning(2, 0)
    assert torch.isfinite(y).all() and torch.isfinite(y_phase).all()
    scale = max(1.0, yd.abs().max().item())
    e_direct = (y - yd).abs().max().item() / scale
    e_f64 = (y.cpu().double() - ref).abs().max().item() / scale
    e_phase = (y - y_phase).abs().max().item() / scale
    is_packed = tiles(H, W, d, m, True) < tiles(H, W, d, m, False)
    print(f"packed winograd m={m} {case}: tiles {tiles(H, W, d, m, False)} -> {tiles(H, W, d, m, True)}, vs direct {e_direct:.2e}, "
          f"vs float64 {e_f64:.2e}, vs per-phase {e_phase:.2e}")
    assert e_direct < tol
    assert e_f64 < tol
    assert (y_phase.cpu().double() - ref).abs().max().item() / scale < tol
    assert e_phase < 1e-5
    # Packing moves a pixel to another position of another tile: other roundings, other bits.  The one exception is F(2x2) on a map
    # whose phases are single pixels on both axes (d >= H, W): a pixel then sits in even slots only - position 0 of its tile, zeros
    # around it, exactly as in a tile of its own - and the next phase's pixel in the tile's halo slot feeds position 3 of the
    # transformed patch, which the outputs of position 0 (A^T row 0: M0 + M1 + M2) do not read.  There the bits must NOT move.
    same_arithmetic = m == 2 and d >= H and d >= W
    if is_packed and not same_arithmetic:
        assert not torch.equal(y, y_phase)
    else:
        assert torch.equal(y, y_phase)
    assert torch.equal(y, y_again)


def test_cases_exercise_the_axis_rules():
    """the geometries above do what their comments say (F(4x4))"""
    assert axis_tiles(30, 6, 4) == (12, 9) and axis_tiles(40, 6, 4) == (12, 12)
    assert axis_tiles(30, 8, 4) == (8, 10) and axis_tiles(40, 8, 4) == (16, 12)
    assert min(axis_tiles(23, 4, 4)) < axis_tiles(23, 4, 4)[0] or min(axis_tiles(37, 4, 4)) < axis_tiles(37, 4, 4)[0]
    assert tiles(7, 9, 12, 4, True) < tiles(7, 9, 12, 4, False)
    assert tiles(13, 5, 3, 4, True) < tiles(13, 5, 3, 4, False)
    assert tiles(5, 6, 8, 4, True) < tiles(5, 6, 8, 4, False)
    # the table of the 30x40 and 45x80 maps
    assert [(tiles(30, 40, d, 4, False), tiles(30, 40, d, 4, True)) for d in (2, 4, 8, 6, 12)] == [(80, 80), (96, 88), (128, 96), (144, 108), (144, 132)]
    assert [(tiles(45, 80, d, 4, False), tiles(45, 80, d, 4, True)) for d in (8, 6, 12)] == [(384, 286), (288, 264), (288, 276)]


# ---------------------------------------------------------------------------------------------------------------- network level
H96, W128, N96 = 96, 128, 5


def _engine96(pack, max_batch, sd):
    """96x128: res5 and the ASPP work on a 6x8 map.  Key 6 = 2 sends that map to Winograd; key 8 = 600 lets its dilated layers qualify at
    all (on 6x8 their per-phase tiles are mostly padding: res5.2.conv2, d = 8, executes 2.4x and ASPP d = 12 5.3x the direct multiplies
    as F(2x2)) - with them res5.2.conv2 has packed rows and ASPP convs.2, whose output transform accumulates GroupNorm sums, packs both axes."""
    eng = engine.Engine(engine.make_config(H96, W128, max_batch=max_batch, max_instances=N96), "cuda:0")
    eng.set_option(6, 2)
    eng.set_option(8, 600)
    eng.set_option(51, pack)
    eng.load_state_dict(sd)
    return eng


@pytest.fixture(scope="module")
def net96():
    sd = arch.init_state_dict(seed=3, loud_heads=True, center_bias=-1.6)
    batch = synth.make_batch(31, 3, H96, W128, N96)
    bgr, dep, masks = (torch.from_numpy(batch[k]).cuda() for k in ("rgb", "depth", "masks"))
    engs = {pack: _engine96(pack, 3, sd) for pack in (1, 0)}
    offs = engs[1].encode(masks)
    out = {pack: e.forward(bgr, dep, offs).clone() for pack, e in engs.items()}
    torch.cuda.synchronize()
    yield {"engs": engs, "in": (bgr, dep, offs), "out": out}
    for e in engs.values():
        e.close()


def test_network_packed_vs_per_phase(net96):
    """GroupNorm sums that counted a separator slot, or a separator that entered the next layer as a pixel, would show here"""
    a, b = net96["out"][1], net96["out"][0]
    engs = net96["engs"]
    # the two plans differ in their tiles, not in their layers
    assert engs[1].forward_flops() == engs[0].forward_flops()
    assert engs[1].forward_flops_padding() < engs[0].forward_flops_padding()
    assert engs[1].forward_flops_executed() < engs[0].forward_flops_executed()
    assert float(a[:, 0].abs().max()) > 0.5                      # the heads are loud
    d = (a - b).abs()
    errs = (float(d[:, :2].max()), float(d[:, 2:4].max()) / 4, float(d[:, 4:].max()))     # head units: the offsets are emitted x4
    print(f"network key 51 = 1 against 0: fg / centre {errs[0]:.2e}, offset / 4 {errs[1]:.2e}, error classes {errs[2]:.2e}")
    assert max(errs) < 1e-4
    assert not torch.equal(a, b)


def test_network_packed_frame_in_batch_is_bit_equal_to_alone(net96):
    """The tiling is a function of (H, W, d, m), never of the batch: frame 1 of a batch of 3 has the bits of the same frame alone.
    The number of K partitions of a GEMM launch does follow the batch (DECISIONS.md, "One algorithm per layer, whatever the batch": a
    re-association of the same fp32 sum, the one per-launch choice), so it is pinned to one partition for the comparison (launch-time key 3):
    unpinned, this frame differs from itself alone by 3.2e-5 with the plan of the defaults, 5.2e-5 with key 6 = 2 and 4.8-6.2e-5 with
    keys 6 = 2, 8 = 600 - the same figures with key 51 = 0, whose bits are those before the key existed; pinned, by 0 with either value."""
    bgr, dep, offs = net96["in"]
    for pack in (1, 0):
        eng = net96["engs"][pack]
        eng.set_option(3, 1)
        try:
            full = eng.forward(bgr, dep, offs).clone()
            alone = eng.forward(bgr[1:2].contiguous(), dep[1:2].contiguous(), offs[1:2].contiguous())
            again = eng.forward(bgr, dep, offs)
            torch.cuda.synchronize()
        finally:
            eng.set_option(3, 0)
        diff = float((alone[0] - full[1]).abs().max())
        print(f"key 51 = {pack}: frame 1 of 3 against the frame alone: max abs difference {diff:.3e}")
        assert torch.equal(alone[0], full[1])
        assert torch.equal(again, full)                              # and from run to run
    again = net96["engs"][1].forward(bgr, dep, offs)
    assert torch.equal(again, net96["out"][1])                       # run to run with the launch rules of the defaults too


def test_network_packed_hipgraph_equals_eager(net96):
    eng = net96["engs"][1]
    bgr, dep, offs = net96["in"]
    logits = torch.zeros_like(net96["out"][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.forward(bgr, dep, offs, logits)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.forward(bgr, dep, offs, logits)
    logits.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(logits, net96["out"][1])


# ---------------------------------------------------------------------------------------------------------------- accounting
def test_profiler_flops_follow_the_tiles():
    """640x480, one frame, exact fp32: the FLOPs the stage profiler reports for the position GEMMs, and the plan's padding figure, move by
    exactly the tiles that packing removes.  The four layers on the 30x40 map whose tiling changes, all F(4x4) (36 GEMMs per tile set):
    res5.1.conv2 (d = 4) and res5.2.conv2 (d = 8), 512 -> 512 channels in both streams; ASPP convs.1 (d = 6) and convs.2 (d = 12), 2048 -> 256."""
    h, w = 480, 640
    sd = arch.init_state_dict(seed=1)
    batch = synth.make_batch(5, 1, h, w, 6)
    bgr, dep, masks = (torch.from_numpy(batch[k]).cuda() for k in ("rgb", "depth", "masks"))
    got = {}
    for pack in (1, 0):
        eng = engine.Engine(engine.make_config(h, w, max_batch=1, max_instances=6), "cuda:0")
        try:
            eng.set_option(51, pack)
            eng.load_state_dict(sd)
            offs = eng.encode(masks)
            eng.forward(bgr, dep, offs)
            eng.profile_begin()
            eng.forward(bgr, dep, offs)
            stages = eng.profile_end()
            got[pack] = (stages["wino_gemm"]["flops"], eng.forward_flops_padding(), eng.forward_flops_executed(), stages["wino_gemm"]["launches"])
        finally:
            eng.close()
    layers = [(2, 512, 512, 4), (2, 512, 512, 8), (1, 2048, 256, 6), (1, 2048, 256, 12)]      # streams, Cin, Cout, d
    gemm = lambda pack: sum(2.0 * 36 * g * tiles(30, 40, d, 4, pack) * cin * cout for g, cin, cout, d in layers)
    assert [tiles(30, 40, d, 4, False) - tiles(30, 40, d, 4, True) for _, _, _, d in layers] == [8, 32, 36, 12]
    saved = gemm(False) - gemm(True)
    print(f"wino_gemm flops {got[0][0]:.6e} -> {got[1][0]:.6e} (expected drop {saved:.6e}); padding {got[0][1]:.6e} -> {got[1][1]:.6e}")
    assert got[1][3] == got[0][3]                                   # the same launches
    assert got[0][0] - got[1][0] == pytest.approx(saved, rel=1e-9)
    # the ratio of the tile sums: the unchanged layers' share is what key 51 = 0 reports beyond the four layers
    rest = got[0][0] - gemm(False)
    assert rest > 0
    assert got[1][0] / got[0][0] == pytest.approx((rest + gemm(True)) / (rest + gemm(False)), rel=1e-9)
    assert got[0][1] - got[1][1] == pytest.approx(saved, rel=1e-9)      # quber_forward_flops_padding drops by the same multiplies
    assert got[0][2] - got[1][2] == pytest.approx(saved, rel=1e-9)      # ... and so does what the forward executes
