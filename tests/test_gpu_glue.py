"""GPU: every glue kernel of csrc/elementwise.hip on its own, in every form the plan launches it - fp32 and fp16 storage, the 16-byte
and the 8-byte fp16 instantiation, channel slices of wider buffers (cs != C), several launch groups (gs) and a batch below the
capacity the strides were computed from - against the float64 restatements of oracle/glue_np.py.

Every destination is allocated wider than the slice written and pre-filled with a sentinel byte; every test asserts that the bytes
outside the slice come back unchanged (neighbouring channels, planes of q no head owns, frames B .. Bcap - 1).

Bounds (from the arithmetic, not from a run):
  fp32 output        rtol 1e-5, atol 2e-6 against float64 (the bar of test_groupnorm_bilinear_maxpool_vs_torch), unless a test says otherwise
  fp16 storage       the kernels compute in fp32 and round once: 2^-11 |ref| + 2^-25 + the fp32 bound
  fp16 against fp32  contraction is off (-ffp-contract=off), so the fp16 kernel's output is bit-equal to the round-to-nearest-even fp16 of
                     the fp32 kernel's output on the same inputs widened to fp32
  max-pool, copy     bit-exact; add = (a.f32 + b.f32) rounded to the storage type; fp32 preprocess = (f32(u8) - mean) / std in float32"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import glue_np as G
from quber_amd import _lib

pytestmark = pytest.mark.gpu

SENT = 0xA5
F32, F16, F64 = np.float32, np.float16, np.float64


def np_dt(es):
    return F32 if es == 4 else F16


def uint_of(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def upload(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda()


def ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def bound32(ref):
    return 1e-5 * np.abs(ref) + 2e-6


def bound16(ref, b32):
    return 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + b32


def assert_within(got, ref, bound, what):
    err = np.abs(got.astype(F64) - ref)
    bound = np.broadcast_to(bound, err.shape)
    bad = err > bound
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0      # (a zero bound: an exact zero is expected)
    print(f"{what}: max error {err.max():.3e}, {ratio:.3f} of the bound")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outside the bound, worst {ratio:.3f}x at {np.argwhere(bad)[0]}"


def assert_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    same = uint_of(np.ascontiguousarray(got)) == uint_of(np.ascontiguousarray(want))
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} elements differ in bits, first at {np.argwhere(~same)[0]}"


class Slab:
    """A buffer [G][Bcap][H][W][cs] of fp32 / fp16 and the view of channels c0 .. c0 + C of its frames 0 .. B - 1 (gs from the capacity).
    A destination is filled with the sentinel byte; a source with values far outside the data (1e3 +- 50) that a kernel must not read."""

    def __init__(self, es, G_, Bcap, H, W, cs, c0, C_, rng=None):
        self.es, self.shape, self.c0, self.C, self.cs = es, (G_, Bcap, H, W, cs), c0, C_, cs
        self.gs = Bcap * H * W * cs
        n = G_ * Bcap * H * W * cs
        if rng is None:
            self.host = np.full(n * es, SENT, np.uint8).view(np_dt(es)).reshape(self.shape)
        else:
            self.host = (rng.standard_normal(n) * 50 + 1000).astype(np_dt(es)).reshape(self.shape)
        self.dev = None

    def put(self, data):
        """data [G][B][H][W][C] -> the view; uploads"""
        self.host[:, :data.shape[1], :, :, self.c0:self.c0 + self.C] = data
        return self.up()

    def up(self):
        self.dev = upload(self.host)
        return self

    @property
    def p(self):
        return ptr(self.dev, self.c0 * self.es)

    def fetch(self, B):
        """the view's frames 0 .. B - 1 after the launch; asserts that every byte outside them is unchanged"""
        torch.cuda.synchronize()
        a = self.dev.cpu().numpy().view(np_dt(self.es)).reshape(self.shape)
        outside = np.ones(self.shape, bool)
        outside[:, :B, :, :, self.c0:self.c0 + self.C] = False
        assert np.array_equal(uint_of(a)[outside], uint_of(self.host)[outside]), "bytes outside the destination slice were written"
        inside = a[:, :B, :, :, self.c0:self.c0 + self.C].copy()
        return inside


def guarded(n, dtype, guard=64):
    """device buffer of n elements between two sentinel guards of `guard` elements; returns (tensor, byte offset of the payload, checker)"""
    es = np.dtype(dtype).itemsize
    t = upload(np.full((n + 2 * guard) * es, SENT, np.uint8))

    def payload():
        torch.cuda.synchronize()
        a = t.cpu().numpy()
        assert (a[:guard * es] == SENT).all() and (a[(guard + n) * es:] == SENT).all(), "bytes around the destination were written"
        return a[guard * es:(guard + n) * es].view(dtype).copy()
    return t, guard * es, payload


# ------------------------------------------------------------------------------------------------------------------------------------
# GroupNorm

def gn_paths(lib, HW, C_, B, G_, V, stats):
    """Which parts of gn_stats_kernel (V = 4) / gn_apply_kernel<T, V> a tensor reaches, from the library's own gn_pixels_per_block and the
    kernels' loop bounds: a lane (row, column) walks its chunk [p0, p1) four pixels in flight (`pix + 3 * rows < p1`), then one at a time."""
    ppb = lib.quber_debug_gn_pixels_per_block(HW, C_, B, G_, 1 if stats else 0)
    cols = C_ // V
    colsper = min(cols, 256)
    rows = 256 // colsper
    got = set()
    for p0 in range(0, HW, ppb):
        p1 = min(HW, p0 + ppb)
        for row in range(rows):
            pix = p0 + row
            while pix + 3 * rows < p1:
                got.add("loop")
                pix += 4 * rows
            if pix < p1:
                got.add("tail")
    if HW > ppb:
        got.add("chunks")
    if HW > ppb and HW % ppb:
        got.add("partial")
    if cols > colsper:
        got.add("passes")
    if rows * colsper < 256 or cols % colsper:
        got.add("idle")
    return got


# (id, es, C, groups, G, B, Bcap, H, W, (in_cs - C, in_c0), (out_cs - C, out_c0), relu, V of the apply kernel, paths the STATS pass must reach,
#  paths the APPLY pass must reach) - asserted against gn_paths before anything is launched.
#   loop / tail = the 4-in-flight loop / the one-at-a-time tail run; chunks = more than one block per frame, partial = a shorter last one;
#   passes = a second column pass (C / V > 256); idle = lanes without a column (256 no multiple of the row width, or a ragged last pass)
GN_CASES = [
    # fp32, gn_apply_kernel<float, 4>
    ("f32-c32-one-channel-per-group", 4, 32, 32, 1, 3, 3, 17, 23, (0, 0), (0, 0), 1, 4, {"tail", "chunks", "partial"}, {"tail", "chunks", "partial"}),
    ("f32-c64-two-per-group", 4, 64, 32, 1, 2, 2, 8, 8, (0, 0), (0, 0), 0, 4, {"tail"}, {"tail", "chunks"}),
    ("f32-c128", 4, 128, 32, 1, 2, 2, 9, 11, (0, 0), (0, 0), 1, 4, {"tail", "chunks", "partial"}, {"tail", "chunks", "partial"}),
    ("f32-c256-rows4-loop-and-tail", 4, 256, 32, 1, 2, 2, 96, 128, (0, 0), (0, 0), 1, 4, {"loop", "chunks"}, {"loop", "tail", "chunks"}),
    ("f32-c320-cpg10-idle-lanes", 4, 320, 32, 1, 3, 3, 5, 7, (0, 0), (0, 0), 0, 4, {"idle", "tail"}, {"idle", "tail"}),
    ("f32-c2048-two-column-passes", 4, 2048, 32, 1, 1, 1, 3, 5, (0, 0), (0, 0), 1, 4, {"passes", "loop", "tail", "partial"}, {"passes", "loop", "tail", "partial"}),
    ("f32-c1280-ragged-second-pass", 4, 1280, 32, 1, 2, 2, 3, 5, (0, 0), (0, 0), 1, 4, {"passes", "idle", "loop", "tail"}, {"passes", "idle", "loop", "tail"}),
    ("f32-hw6", 4, 32, 32, 1, 2, 2, 2, 3, (0, 0), (0, 0), 1, 4, {"tail"}, {"tail"}),
    ("f32-c32-stats-loop-tail-partial", 4, 32, 32, 1, 1, 1, 97, 131, (0, 0), (0, 0), 0, 4, {"loop", "tail", "chunks", "partial"}, {"tail", "chunks", "partial"}),
    ("f32-two-groups-below-capacity-slices", 4, 64, 32, 2, 2, 3, 30, 41, (16, 4), (32, 8), 1, 4, {"tail", "chunks", "partial"}, {"tail", "chunks", "partial"}),
    # fp16, gn_apply_kernel<half_t, 8> (C, both cs and gs multiples of 8, both views 16-byte aligned)
    ("f16-wide-two-groups-slices", 2, 64, 32, 2, 2, 3, 30, 41, (16, 8), (32, 16), 1, 8, {"tail", "chunks", "partial"}, {"tail", "chunks", "partial"}),
    ("f16-wide-c2048-rows1", 2, 2048, 32, 1, 1, 1, 3, 5, (0, 0), (0, 0), 0, 8, {"passes", "loop", "tail", "partial"}, {"loop", "tail", "partial"}),
    ("f16-wide-c128-rows16-loop-and-tail", 2, 128, 32, 2, 2, 2, 97, 128, (0, 0), (0, 0), 1, 8, {"loop", "chunks"}, {"loop", "tail", "chunks", "partial"}),
    ("f16-wide-c320-lane-spans-groups", 2, 320, 32, 1, 2, 2, 5, 7, (0, 0), (0, 0), 1, 8, {"idle", "tail"}, {"idle", "tail"}),
    # fp16, gn_apply_kernel<half_t, 4>: C % 8 != 0 (12 channels in 3 groups), or a view that starts 4 channels = 8 bytes into its buffer
    ("f16-fallback-c12", 2, 12, 3, 2, 2, 3, 9, 11, (0, 0), (4, 0), 1, 4, {"tail"}, {"tail", "chunks", "partial"}),
    ("f16-fallback-8-bytes-in", 2, 64, 32, 1, 2, 2, 9, 11, (8, 4), (8, 4), 0, 4, {"tail"}, {"tail", "chunks", "partial"}),
    ("f16-fallback-c256-rows4-loop-and-tail", 2, 256, 32, 1, 2, 2, 96, 128, (0, 0), (8, 4), 1, 4, {"loop", "chunks"}, {"loop", "tail", "chunks"}),
]


def gn_launch(lib, xs, ys, es, B, H, W, C_, G_, groups, stats_p, gam_d, bet_d, relu, zero=1, do_stats=True):
    if do_stats:
        _lib.check(lib.quber_op_gn_stats(xs.p, xs.cs, xs.gs, xs.es, B, H, W, C_, G_, groups, stats_p, zero, stream()))
    _lib.check(lib.quber_op_gn_apply(xs.p, xs.cs, xs.gs, xs.es, ys.p, ys.cs, ys.gs, ys.es, B, H, W, C_, G_, groups, stats_p, ptr(gam_d), ptr(bet_d),
                                     C_, 1e-5, relu, stream()))


@pytest.mark.parametrize("case", GN_CASES, ids=[c[0] for c in GN_CASES])
def test_groupnorm(case):
    name, es, C_, groups, G_, B, Bcap, H, W, (in_pad, in_c0), (out_pad, out_c0), relu, V, want_stats, want_apply = case
    lib = _lib.load()
    got_stats, got_apply = gn_paths(lib, H * W, C_, B, G_, 4, True), gn_paths(lib, H * W, C_, B, G_, V, False)
    assert want_stats <= got_stats and want_apply <= got_apply, (name, got_stats, got_apply)
    if H * W < 8:
        assert "chunks" not in got_apply
    # the launcher takes the 16-byte instantiation exactly when ...
    wide = es == 2 and C_ % 8 == 0 and (C_ + in_pad) % 8 == 0 and (C_ + out_pad) % 8 == 0 and in_c0 % 8 == 0 and out_c0 % 8 == 0
    assert (V == 8) == wide, name
    rng = np.random.default_rng(len(name) + C_ + H)
    x = (rng.standard_normal((G_, B, H, W, C_)) * 3 + 1).astype(np_dt(es))
    gam = (rng.random((G_, C_)) + 0.5).astype(F32)          # distinct per launch group (param_gs = C)
    bet = rng.standard_normal((G_, C_)).astype(F32)
    xs = Slab(es, G_, Bcap, H, W, C_ + in_pad, in_c0, C_, rng).put(x)
    ys = Slab(es, G_, Bcap, H, W, C_ + out_pad, out_c0, C_).up()
    gam_d, bet_d = upload(gam), upload(bet)
    n_stats = G_ * B * groups * 2
    stats_t, stats_off, stats_get = guarded(n_stats, F64, guard=16)
    gn_launch(lib, xs, ys, es, B, H, W, C_, G_, groups, ptr(stats_t, stats_off), gam_d, bet_d, relu)
    y = ys.fetch(B)
    stats = stats_get().reshape(G_, B, groups, 2)
    n = H * W * (C_ // groups)
    ref = np.stack([G.group_norm(x[g], groups, gam[g], bet[g], 1e-5, bool(relu)) for g in range(G_)])
    sums = np.stack([G.group_sums(x[g], groups) for g in range(G_)])
    # fp64 sums of n terms in some order: n roundings of at most 2^-53 of the running sum of magnitudes, on either side
    xa = np.abs(x.astype(F64)).reshape(G_, B, H * W, groups, C_ // groups)
    mags = np.stack([xa.sum(axis=(2, 4)), (xa * xa).sum(axis=(2, 4))], axis=-1)
    assert (np.abs(stats - sums) <= 2 * n * 2.0 ** -53 * mags).all(), name
    b32 = bound32(ref)
    assert_within(y, ref, b32 if es == 4 else bound16(ref, b32), f"groupnorm {name}")
    if es == 2:
        # the same statistics, the fp32 kernel on the widened input: the fp16 kernel's output is its RNE fp16
        xw = Slab(4, G_, Bcap, H, W, C_ + in_pad, in_c0, C_, rng).put(x.astype(F32))
        yw = Slab(4, G_, Bcap, H, W, C_ + out_pad, out_c0, C_).up()
        gn_launch(lib, xw, yw, 4, B, H, W, C_, G_, groups, ptr(stats_t, stats_off), gam_d, bet_d, relu, do_stats=False)
        assert_bits(y, yw.fetch(B).astype(F16), f"groupnorm {name}: fp16 kernel against the fp32 kernel")


def test_groupnorm_accumulates_unless_told_to_zero():
    """zero = false on a pre-cleared accumulator gives the sums of zero = true (the order of the fp64 atomics is free: equal to the rounding
    of the sums, and the normalised output to the usual bound); a second zero = false pass doubles them."""
    lib = _lib.load()
    es, C_, G_, B, H, W = 4, 64, 2, 2, 9, 11
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((G_, B, H, W, C_)) * 3 + 1).astype(F32)
    gam, bet = (rng.random((G_, C_)) + 0.5).astype(F32), rng.standard_normal((G_, C_)).astype(F32)
    xs = Slab(es, G_, B, H, W, C_, 0, C_, rng).put(x)
    gam_d, bet_d = upload(gam), upload(bet)
    ref = np.stack([G.group_norm(x[g], 32, gam[g], bet[g], 1e-5, True) for g in range(G_)])
    sums = np.stack([G.group_sums(x[g], 32) for g in range(G_)])
    tol = H * W * 2 * 2.0 ** -53 * np.abs(sums).max() * 4
    dirty = upload(np.full(G_ * B * 32 * 2, 1e30, F64))
    ys = Slab(es, G_, B, H, W, C_, 0, C_).up()
    gn_launch(lib, xs, ys, es, B, H, W, C_, G_, 32, ptr(dirty), gam_d, bet_d, 1, zero=1)
    assert_within(ys.fetch(B), ref, bound32(ref), "zero = true on a dirty accumulator")
    s_true = dirty.cpu().numpy().view(F64).reshape(sums.shape)
    clean = upload(np.zeros(G_ * B * 32 * 2, F64))
    ys = Slab(es, G_, B, H, W, C_, 0, C_).up()
    gn_launch(lib, xs, ys, es, B, H, W, C_, G_, 32, ptr(clean), gam_d, bet_d, 1, zero=0)
    assert_within(ys.fetch(B), ref, bound32(ref), "zero = false on a cleared accumulator")
    s_false = clean.cpu().numpy().view(F64).reshape(sums.shape)
    assert np.abs(s_true - sums).max() <= tol and np.abs(s_false - sums).max() <= tol
    _lib.check(lib.quber_op_gn_stats(xs.p, xs.cs, xs.gs, es, B, H, W, C_, G_, 32, ptr(clean), 0, stream()))
    torch.cuda.synchronize()
    assert np.abs(clean.cpu().numpy().view(F64).reshape(sums.shape) - 2 * sums).max() <= 2 * tol


def test_groupnorm_offset_input_against_torch_float32_error():
    """mean 100, std 1: `x * scale + (beta - mean * scale)` cancels two numbers of ~100 * scale, so ANY float32 implementation of torch's
    CPU form is ulp(100) ~ 8e-6 per rounding away from float64 and the 2e-6 bar cannot hold.  The yardstick is measured here instead: the
    kernel's maximum error may be at most twice that of torch's own float32 group_norm on the same input (two correct implementations
    of one error model differ in their maxima; float32 moments or a float32 variance miss it by orders of magnitude)."""
    lib = _lib.load()
    B, H, W, C_ = 2, 30, 40, 64
    rng = np.random.default_rng(100)
    x = (rng.standard_normal((1, B, H, W, C_)) + 100).astype(F32)
    gam, bet = (rng.random((1, C_)) + 0.5).astype(F32), rng.standard_normal((1, C_)).astype(F32)
    xs = Slab(4, 1, B, H, W, C_, 0, C_, rng).put(x)
    ys = Slab(4, 1, B, H, W, C_, 0, C_).up()
    gam_d, bet_d = upload(gam), upload(bet)
    stats = upload(np.zeros(B * 64, F64))
    gn_launch(lib, xs, ys, 4, B, H, W, C_, 1, 32, ptr(stats), gam_d, bet_d, 0)
    y = ys.fetch(B)[0]
    ref = G.group_norm(x[0], 32, gam[0], bet[0], 1e-5)
    # (a CONTIGUOUS NCHW tensor: torch's channels-last CPU kernel takes its variance as E[x^2] - E[x]^2 in float32 and is 1e-2 away on this
    # input - a yardstick that would let exactly the float32 variance pass which this test is there to catch)
    tor = torch.nn.functional.group_norm(torch.from_numpy(x[0]).permute(0, 3, 1, 2).contiguous(), 32, torch.from_numpy(gam[0]),
                                         torch.from_numpy(bet[0]), 1e-5)
    e_torch = float(np.abs(tor.permute(0, 2, 3, 1).numpy().astype(F64) - ref).max())
    e_form = float(np.abs(G.group_norm(x[0], 32, gam[0], bet[0], 1e-5, torch_f32_form=True).astype(F64) - ref).max())
    e_hip = float(np.abs(y.astype(F64) - ref).max())
    print(f"groupnorm, mean 100 std 1: kernel {e_hip:.3e}, torch float32 {e_torch:.3e}, float32 restatement {e_form:.3e} from float64; "
          f"ratio kernel / torch {e_hip / e_torch:.3f}")
    assert e_hip <= 2 * e_torch


# ------------------------------------------------------------------------------------------------------------------------------------
# max-pool

# (id, es, C, G, B, Bcap, H, W, (in_cs - C, in_c0), (out_cs - C, out_c0), all negative, V)
#   V = channels per lane: maxpool_kernel<float, 4>, <half_t, 8> (wide), <half_t, 4> (C % 8 != 0 or a view 8 bytes into its buffer);
#   OW * C / V lanes per output row: below 256 = one partly idle block, just above a multiple of 256 = a last block with few lanes
MP_CASES = [
    ("f32-odd", 4, 8, 1, 2, 2, 11, 15, (0, 0), (0, 0), True, 4),                     # 8 * 2 = 16 lanes per row; last window row / column outside
    ("f32-even", 4, 8, 1, 1, 1, 10, 14, (0, 0), (0, 0), False, 4),
    ("f32-one-row", 4, 4, 1, 1, 1, 1, 9, (0, 0), (0, 0), True, 4),
    ("f32-one-column", 4, 4, 1, 1, 1, 7, 1, (0, 0), (0, 0), True, 4),
    ("f32-257-lanes", 4, 4, 1, 1, 1, 3, 513, (0, 0), (0, 0), True, 4),               # OW = 257, C / 4 = 1: 256 + 1
    ("f32-528-lanes", 4, 64, 1, 1, 1, 5, 65, (0, 0), (0, 0), False, 4),              # OW = 33, C / 4 = 16: 2 * 256 + 16
    ("f32-two-groups-below-capacity-slices", 4, 16, 2, 2, 3, 11, 15, (8, 4), (16, 8), True, 4),
    ("f16-wide", 2, 16, 1, 2, 2, 11, 15, (0, 0), (0, 0), True, 8),
    ("f16-wide-two-groups-slices-264-lanes", 2, 64, 2, 2, 3, 6, 65, (16, 8), (32, 16), True, 8),      # OW = 33, C / 8 = 8: 256 + 8
    ("f16-fallback-c12", 2, 12, 2, 2, 3, 11, 15, (0, 0), (4, 0), True, 4),
    ("f16-fallback-8-bytes-in", 2, 16, 1, 2, 2, 10, 14, (8, 4), (8, 4), False, 4),
    ("f16-fallback-one-pixel", 2, 4, 1, 1, 1, 1, 1, (0, 0), (0, 0), True, 4),
]


@pytest.mark.parametrize("case", MP_CASES, ids=[c[0] for c in MP_CASES])
def test_maxpool(case):
    name, es, C_, G_, B, Bcap, H, W, (in_pad, in_c0), (out_pad, out_c0), neg, V = case
    lib = _lib.load()
    wide = es == 2 and C_ % 8 == 0 and (C_ + in_pad) % 8 == 0 and (C_ + out_pad) % 8 == 0 and in_c0 % 8 == 0 and out_c0 % 8 == 0
    assert (V == 8) == wide
    rng = np.random.default_rng(len(name) + H * W)
    x = rng.standard_normal((G_, B, H, W, C_))
    x = (-1 - np.abs(x) if neg else x).astype(np_dt(es))      # all negative: a zero-padded or zero-initialised maximum would show
    OH, OW = (H + 1) // 2, (W + 1) // 2
    xs = Slab(es, G_, Bcap, H, W, C_ + in_pad, in_c0, C_, rng).put(x)
    ys = Slab(es, G_, Bcap, OH, OW, C_ + out_pad, out_c0, C_).up()
    _lib.check(lib.quber_op_maxpool_view(xs.p, xs.cs, xs.gs, es, ys.p, ys.cs, ys.gs, es, B, H, W, C_, G_, stream()))
    ref = np.stack([G.maxpool3x3s2(x[g]) for g in range(G_)])
    assert_bits(ys.fetch(B), ref, f"maxpool {name}")


# ------------------------------------------------------------------------------------------------------------------------------------
# bilinear resize

# (id, C, B, H, W, OH, OW, (in_cs - C, in_c0), (out_cs - C, out_c0)); every case runs as bilinear_kernel<float, 4> and in fp16 - as
# <half_t, 8> where C and both slices allow 16-byte accesses, else as <half_t, 4>
BL_CASES = [
    ("broadcast-1x1-to-30x40-into-1024", 256, 2, 1, 1, 30, 40, (0, 0), (1024, 1024)),      # the ASPP pooling branch: channels 1024 .. 1279 of 1280
    ("x2-into-32", 32, 2, 15, 20, 30, 40, (0, 0), (64, 32)),
    ("x4-into-64", 8, 1, 8, 10, 32, 40, (8, 8), (120, 64)),
    ("7x9-to-10x31", 8, 2, 7, 9, 10, 31, (0, 0), (8, 0)),                                 # no integer ratio: fractional weights, clamped last row
    ("identity", 8, 1, 6, 5, 6, 5, (0, 0), (0, 0)),
    ("down-9x7-to-4x3", 16, 1, 9, 7, 4, 3, (0, 0), (0, 0)),
    ("c4-fallback", 4, 2, 7, 9, 10, 31, (0, 0), (4, 0)),                                   # fp16: C % 8 != 0
    ("c12-fallback-1x1", 12, 1, 1, 1, 5, 6, (0, 0), (4, 4)),
    ("8-bytes-in-fallback", 16, 1, 15, 20, 30, 40, (8, 4), (16, 4)),                       # fp16: both views start 8 bytes into their buffers
    ("300-lanes", 16, 1, 3, 4, 6, 75, (0, 0), (0, 0)),                                     # OW * C / 4 = 300: a second, partly idle block (fp16 wide: 150)
]


@pytest.mark.parametrize("case", BL_CASES, ids=[c[0] for c in BL_CASES])
def test_bilinear(case):
    name, C_, B, H, W, OH, OW, (in_pad, in_c0), (out_pad, out_c0) = case
    lib = _lib.load()
    rng = np.random.default_rng(len(name) + OH * OW)
    x16 = rng.standard_normal((1, B, H, W, C_)).astype(F16)
    out = {}
    for run, es, x in (("f32", 4, rng.standard_normal((1, B, H, W, C_)).astype(F32)), ("f16 widened", 4, x16.astype(F32)), ("f16", 2, x16)):
        xs = Slab(es, 1, B, H, W, C_ + in_pad, in_c0, C_, rng).put(x)
        ys = Slab(es, 1, B, OH, OW, C_ + out_pad, out_c0, C_).up()
        _lib.check(lib.quber_op_bilinear_view(xs.p, xs.cs, es, ys.p, ys.cs, es, B, H, W, C_, OH, OW, stream()))
        out[run] = ys.fetch(B)[0]
        ref = G.bilinear(x[0], OH, OW)
        b32 = bound32(ref)
        assert_within(out[run], ref, b32 if es == 4 else bound16(ref, b32), f"bilinear {name}, {run}")
    assert_bits(out["f16"], out["f16 widened"].astype(F16), f"bilinear {name}: fp16 kernel against the fp32 kernel")


# ------------------------------------------------------------------------------------------------------------------------------------
# global average pool

@pytest.mark.parametrize("es", [4, 2], ids=["f32", "f16"])
def test_avgpool(es):
    """HW 1 / 15 (tail only), 128 (one trip of the 8-in-flight loop, no tail), 129 and 300 (loop and tail); C 4 (one column of a block),
    68 (a second block with one column), 2048 (32 blocks); the source a slice 4 channels into a wider buffer, the means at stride C + 4."""
    lib = _lib.load()
    rng = np.random.default_rng(es)
    B = 2
    for (H, W) in [(1, 1), (3, 5), (8, 16), (3, 43), (15, 20)]:
        for C_ in (4, 68, 2048):
            x = (rng.standard_normal((1, B, H, W, C_)) + 0.5).astype(np_dt(es))
            xs = Slab(es, 1, B, H, W, C_ + 8, 4, C_, rng).put(x)
            ys = Slab(es, 1, B, 1, 1, C_ + 4, 0, C_).up()
            _lib.check(lib.quber_op_avgpool(xs.p, xs.cs, es, ys.p, ys.cs, es, B, H, W, C_, stream()))
            y = ys.fetch(B)[0, :, 0, 0, :]
            ref = G.avgpool(x[0])
            # fp64 sums divided in fp64, rounded once to fp32: the correctly rounded mean or its neighbour
            ulp = np.spacing(np.abs(ref.astype(F32))).astype(F64)
            assert_within(y, ref.astype(F32).astype(F64) if es == 4 else ref, ulp if es == 4 else bound16(ref, ulp), f"avgpool {H}x{W}x{C_} es {es}")


# ------------------------------------------------------------------------------------------------------------------------------------
# predictors

EXPF_ULP = 1.0      # HIP math API: expf, maximum error 1 ulp


def run_predictors(C_, es, heads, B, H, W, q_nch, feat_pad=0, feat_c0=0, w_std=1.5, seed=0):
    """heads: (cout, q_ch0, act, activation channel offset or None).  Returns per head (x, w, bias, logits read back, activations read
    back or None) after asserting that no byte of q / of the activation buffer outside the heads' planes / slices changed."""
    lib = _lib.load()
    rng = np.random.default_rng(seed + C_ + len(heads))
    n = len(heads)
    HW = H * W
    act_cs = 12
    feats, ws, bs, keep = [], [], [], []
    for (cout, q0, act, a0) in heads:
        x = rng.standard_normal((1, B, H, W, C_)).astype(np_dt(es))
        feats.append((x, Slab(es, 1, B, H, W, C_ + feat_pad, feat_c0, C_, rng).put(x)))
        ws.append((rng.standard_normal((cout, C_)) * w_std / math.sqrt(C_)).astype(F32))
        bs.append(rng.standard_normal(cout).astype(F32))
    w_d, b_d = [upload(w) for w in ws], [upload(b) for b in bs]
    q_t, q_off, q_get = guarded(B * q_nch * HW, F32)
    act_t, act_off, act_get = guarded(B * HW * act_cs, np_dt(es))
    PA, IA = C.c_void_p * n, C.c_int32 * n
    feat_a = PA(*[f[1].p.value for f in feats])
    w_a, b_a = PA(*[t.data_ptr() for t in w_d]), PA(*[t.data_ptr() for t in b_d])
    dst_a = PA(*[(act_t.data_ptr() + act_off + a0 * es) if a0 is not None else None for (_, _, _, a0) in heads])
    cout_a, q0_a, act_a = IA(*[h[0] for h in heads]), IA(*[h[1] for h in heads]), IA(*[h[2] for h in heads])
    _lib.check(lib.quber_op_predictors(n, feat_a, w_a, b_a, dst_a, cout_a, q0_a, act_a, C_, C_ + feat_pad, es, B, H, W, ptr(q_t, q_off), q_nch,
                                       act_cs, stream()))
    q = q_get().reshape(B, q_nch, HW)
    a = act_get().reshape(B, HW, act_cs)
    q_owned, a_owned = np.zeros(q_nch, bool), np.zeros(act_cs, bool)
    out = []
    for (cout, q0, act, a0), (x, slab), w, b in zip(heads, feats, ws, bs):
        slab.fetch(B)                                        # (the features are untouched)
        q_owned[q0:q0 + cout] = True
        if a0 is not None:
            a_owned[a0:a0 + cout] = True
        out.append((x[0], w, b, q[:, q0:q0 + cout].reshape(B, cout, H, W), None if a0 is None else a[:, :, a0:a0 + cout].reshape(B, H, W, cout)))
    sent = {4: np.uint32(0xA5A5A5A5), 2: np.uint16(0xA5A5)}
    assert (uint_of(q)[:, ~q_owned] == sent[4]).all(), "a logit plane no head owns was written"
    assert (uint_of(a)[:, :, ~a_owned] == sent[es]).all(), "activation channels no head owns were written"
    return out


def check_predictors(heads, results, es, what):
    for (cout, q0, act, a0), (x, w, b, z, a) in zip(heads, results):
        C_ = x.shape[-1]
        ref = G.predictor_logits(x, w, b)
        # a chain of C fmas and one addition, each rounding at most 2^-24 of a partial sum that never exceeds sum |x_j w_j| + |bias|
        mag = np.einsum("bhwc,kc->bkhw", np.abs(x.astype(F64)), np.abs(w.astype(F64))) + np.abs(b.astype(F64))[None, :, None, None]
        assert_within(z, ref, (C_ + 2) * 2.0 ** -24 * mag, f"{what}: logits of head at plane {q0}")
        if a is None:
            continue
        zk = np.moveaxis(z, 1, -1).astype(F64)                # the kernel's own logits, [B][H][W][cout]
        assert np.abs(zk).max() <= 16
        if act == 2:
            # 1 / (1 + expf(-z)): the negation is exact, expf EXPF_ULP ulp (2^-23 each, its weight e / (1 + e) < 1), the addition and the
            # division 2^-24 each: relative (EXPF_ULP * 2 + 2) * 2^-24, first order - 1 % for the products of these terms
            want = G.sigmoid(zk)
            rel = 1.01 * (2 * EXPF_ULP + 2) * 2.0 ** -24
        else:
            # e_k = expf(z_k - max): the subtraction rounds by |z_k - max| 2^-24 at most, an ABSOLUTE error of the exponent = relative of
            # e_k, plus expf's ulp: eps_k <= d 2^-24 + EXPF_ULP 2^-23 with d = max_k |z_k - max|.  The sum of cout positive terms carries
            # at most the largest eps_k plus cout - 1 additions of 2^-24; the quotient eps_k + that + 2^-24 for the division
            want = G.softmax(zk, -1)
            d = (zk.max(axis=-1, keepdims=True) - zk).max(axis=-1, keepdims=True)
            assert d.max() <= 16
            rel = 1.01 * (2 * (d + 2 * EXPF_ULP) + cout) * 2.0 ** -24
        b32 = rel * want
        assert_within(a, want, b32 if es == 4 else bound16(want, b32), f"{what}: activation of head at plane {q0}")


# (id, C, es, B, H, W, q_nch, (feat_cs - C, feat_c0), heads (cout, first plane, act 0 none / 1 softmax / 2 sigmoid, activation channel offset))
PRED_CASES = [
    ("c32-one-head-plain", 32, 4, 2, 5, 7, 3, (0, 0), [(1, 1, 0, None)]),
    ("c32-three-heads", 32, 4, 2, 9, 11, 9, (8, 4), [(1, 0, 2, 1), (2, 2, 1, 3), (4, 5, 1, 6)]),           # planes 1, 4 and channels 0, 2, 5, 10, 11 unowned
    ("c64-five-heads", 64, 4, 1, 6, 5, 14, (0, 0), [(1, 0, 2, 0), (1, 1, 0, None), (2, 3, 2, 1), (3, 5, 1, 5), (4, 9, 1, 8)]),
    ("c64-three-outputs-offset-9", 64, 4, 2, 3, 3, 3, (4, 0), [(3, 0, 1, 9)]),
    ("f16-c32-three-heads", 32, 2, 2, 9, 11, 9, (8, 4), [(1, 0, 2, 1), (2, 2, 1, 3), (4, 5, 1, 7)]),
    ("f16-c64-two-heads", 64, 2, 1, 6, 5, 8, (0, 0), [(3, 1, 1, 1), (2, 5, 2, 5)]),
]


@pytest.mark.parametrize("case", PRED_CASES, ids=[c[0] for c in PRED_CASES])
def test_predictors(case):
    name, C_, es, B, H, W, q_nch, (pad, c0), heads = case
    check_predictors(heads, run_predictors(C_, es, heads, B, H, W, q_nch, pad, c0), es, name)


def test_predictors_second_grid_stride_trip():
    """2 x 480 x 640 = 614 400 pixels: more than the 2048 x 256 = 524 288 threads a launch is capped at, so 90 112 lanes make a second trip"""
    heads = [(2, 1, 1, 5)]
    check_predictors(heads, run_predictors(32, 4, heads, 2, 480, 640, 4), 4, "predictor, 614400 pixels")


# ------------------------------------------------------------------------------------------------------------------------------------
# logit up-sampling

# (id, nch, h, w, OH, OW, mul_mask, destination offset in floats): upsample_logits_kernel<4> when OW % 4 == 0 and the destination is
# 16-byte aligned, else <1>.  B = 2 and nch > 4 everywhere: frame 1's planes are nch .. 2 nch - 1, the mask is read at plane % nch
UP_CASES = [
    ("scalar-cropped-53x75", 6, 14, 19, 53, 75, 0xC, 0),
    ("vector-full-56x76", 6, 14, 19, 56, 76, 0xC, 0),
    ("vector-cropped-53x72-no-mask", 5, 14, 19, 53, 72, 0x0, 0),
    ("vector-width-but-4-bytes-off", 6, 3, 4, 12, 16, 0xC, 1),
    ("scalar-one-pixel-source", 5, 1, 1, 3, 3, 0x11, 0),
]


@pytest.mark.parametrize("case", UP_CASES, ids=[c[0] for c in UP_CASES])
def test_upsample_logits(case):
    name, nch, h, w, OH, OW, mask, off = case
    lib = _lib.load()
    B = 2
    rng = np.random.default_rng(OH * OW + nch)
    q = rng.standard_normal((B, nch, h, w)).astype(F32)
    q_d = upload(q)
    n = B * nch * OH * OW
    out_t, out_off, out_get = guarded(n + off, F32)
    _lib.check(lib.quber_op_upsample_logits(ptr(q_d), ptr(out_t, out_off + 4 * off), B, nch, h, w, 4, OH, OW, mask, stream()))
    got = out_get()
    assert (uint_of(got[:off]) == np.uint32(0xA5A5A5A5)).all()
    ref = G.upsample_logits(q, 4, OH, OW, mask)
    got = got[off:].reshape(B, nch, OH, OW)
    for b in range(B):
        assert_within(got[b], ref[b], bound32(ref[b]), f"upsample {name}, frame {b}")


def test_upsample_logits_refuses_a_frame_larger_than_the_map():
    lib = _lib.load()
    q_d = upload(np.zeros((1, 2, 3, 4), F32))
    out_t, out_off, out_get = guarded(2 * 13 * 17, F32)
    for (OH, OW) in ((13, 16), (12, 17)):
        with pytest.raises(_lib.QuberError, match="frame larger"):
            _lib.check(lib.quber_op_upsample_logits(ptr(q_d), ptr(out_t, out_off), 1, 2, 3, 4, 4, OH, OW, 0, stream()))
    assert (out_get().view(np.uint32) == 0xA5A5A5A5).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# preprocess

MEAN6 = [103.53, 116.28, 123.675, 127.5, 120.25, 131.0]
STD6 = [1.0, 57.375, 58.395, 127.5, 3.0, 0.7]

# (id, streams, x.C, es, B, Bcap, H, W)
PP_CASES = [
    ("two-streams-below-capacity", 2, 8, 4, 2, 3, 5, 7),
    ("one-stream", 1, 8, 4, 1, 1, 4, 4),
    ("two-streams-16-channels", 2, 16, 4, 1, 2, 6, 5),         # channels 8 .. 15 zero-filled
    ("f16-two-streams-below-capacity", 2, 8, 2, 2, 3, 5, 7),
    ("f16-one-stream-16-channels", 1, 16, 2, 2, 2, 3, 9),
    ("two-streams-614400-pixels", 2, 8, 4, 2, 2, 480, 640),     # more pixels than the 524 288 threads of a capped launch
]


@pytest.mark.parametrize("case", PP_CASES, ids=[c[0] for c in PP_CASES])
def test_preprocess(case):
    name, streams, xc, es, B, Bcap, H, W = case
    lib = _lib.load()
    rng = np.random.default_rng(H * W + xc)
    bgr = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    dep = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8) if streams == 2 else None
    offs = rng.standard_normal((B, 3, H, W)).astype(F32)
    bgr_d, offs_d = upload(bgr), upload(offs)
    dep_d = upload(dep) if streams == 2 else None
    xs = Slab(es, streams, Bcap, H, W, xc, 0, xc).up()
    mean, std = (C.c_float * 6)(*MEAN6), (C.c_float * 6)(*STD6)
    _lib.check(lib.quber_op_preprocess(ptr(bgr_d), ptr(dep_d) if streams == 2 else None, ptr(offs_d), xs.p, xc, es, B, Bcap, H, W, mean, std,
                                       streams, stream()))
    got = xs.fetch(B)
    want = G.preprocess(bgr, dep, offs, MEAN6, STD6, xc, dtype=F32)     # (f32(u8) - mean) / std, each operation rounded to float32
    assert_bits(got, want if es == 4 else want.astype(F16), f"preprocess {name}")
    ref = G.preprocess(bgr, dep, offs, np.array(MEAN6, F32).astype(F64), np.array(STD6, F32).astype(F64), xc)
    b32 = 1.01 * 2.0 ** -23 * np.abs(ref)          # one subtraction and one division, 2^-24 relative each; the offsets are copies
    assert_within(got, ref, b32 if es == 4 else bound16(ref, b32), f"preprocess {name} against float64")


# ------------------------------------------------------------------------------------------------------------------------------------
# add / copy of channel slices

# (id, es, C, B, H, W, (a_cs, a_c0), (b_cs, b_c0), (out_cs, out_c0)): three different strides
AC_CASES = [
    ("f32-strides-24-40-16", 4, 16, 2, 5, 7, (24, 4), (40, 16), (16, 0)),
    ("f32-c4", 4, 4, 1, 3, 3, (8, 4), (12, 0), (20, 12)),
    ("f16-strides-24-40-32", 2, 16, 2, 5, 7, (24, 4), (40, 16), (32, 8)),
    ("f16-c12", 2, 12, 1, 4, 5, (12, 0), (16, 4), (20, 8)),
    ("f32-540000-quads", 4, 12, 2, 300, 300, (12, 0), (16, 4), (20, 8)),      # pixels * C / 4 = 540 000 > 524 288: a second grid-stride trip
]


@pytest.mark.parametrize("case", AC_CASES, ids=[c[0] for c in AC_CASES])
def test_add_and_copy_channels(case):
    name, es, C_, B, H, W, (a_cs, a_c0), (b_cs, b_c0), (o_cs, o_c0) = case
    lib = _lib.load()
    rng = np.random.default_rng(C_ + H)
    a = rng.standard_normal((1, B, H, W, C_)).astype(np_dt(es))
    b = (rng.standard_normal((1, B, H, W, C_)) * 3).astype(np_dt(es))
    sa, sb = Slab(es, 1, B, H, W, a_cs, a_c0, C_, rng).put(a), Slab(es, 1, B, H, W, b_cs, b_c0, C_, rng).put(b)
    so = Slab(es, 1, B, H, W, o_cs, o_c0, C_).up()
    _lib.check(lib.quber_op_add_channels(sa.p, a_cs, es, sb.p, b_cs, es, so.p, o_cs, es, B, H, W, C_, stream()))
    assert_bits(so.fetch(B), (a.astype(F32) + b.astype(F32)).astype(np_dt(es)), f"add {name}")
    so = Slab(es, 1, B, H, W, o_cs, o_c0, C_).up()
    _lib.check(lib.quber_op_copy_channels(sb.p, b_cs, es, so.p, o_cs, es, B, H, W, C_, stream()))
    assert_bits(so.fetch(B), b, f"copy {name}")


# ------------------------------------------------------------------------------------------------------------------------------------
# views a launcher refuses

def test_refused_views_return_the_launchers_error():
    """Mixed element types, channel counts and strides that are no multiple of 4 (a half-typed view with cs = 10 would reach the 8-byte
    loads 4 bytes off), a base address off the 4-element boundary: the launcher's error comes back, nothing is launched or written."""
    lib = _lib.load()
    buf_t, off, get = guarded(4096, F32)
    p, st = ptr(buf_t, off), stream()
    p2 = ptr(buf_t, off + 4)            # 4 bytes in: off the 16-byte (fp32) and the 8-byte (fp16) boundary
    stats = upload(np.zeros(256, F64))
    E = _lib.QuberError

    def refused(match, rc):
        with pytest.raises(E, match=match):
            _lib.check(rc)

    refused("mixed element types", lib.quber_op_gn_apply(p, 32, 0, 4, p, 32, 0, 2, 1, 2, 2, 32, 1, 32, ptr(stats), p, p, 32, 1e-5, 1, st))
    refused("mixed element types", lib.quber_op_maxpool_view(p, 8, 0, 2, p, 8, 0, 4, 1, 4, 4, 8, 1, st))
    refused("mixed element types", lib.quber_op_bilinear_view(p, 8, 4, p, 8, 2, 1, 2, 2, 8, 4, 4, st))
    refused("mixed element types", lib.quber_op_avgpool(p, 8, 4, p, 8, 2, 1, 2, 2, 8, st))
    refused("mixed element types", lib.quber_op_add_channels(p, 8, 4, p, 8, 2, p, 8, 4, 1, 2, 2, 8, st))
    refused("mixed element types", lib.quber_op_copy_channels(p, 8, 2, p, 8, 4, 1, 2, 2, 8, st))
    for es in (4, 2):
        # C = 6; then cs = 10 at C = 8; then a misplaced base address
        for (c, cs, q) in ((6, 8, p), (8, 10, p), (8, 8, p2)):
            refused("groups of 4|channel/group", lib.quber_op_gn_stats(q, cs, 0, es, 1, 2, 2, c, 1, 2, ptr(stats), 1, st))
            refused("groups of 4|channel/group", lib.quber_op_gn_apply(q, cs, 0, es, p, 8, 0, es, 1, 2, 2, c, 1, 2, ptr(stats), p, p, 8, 1e-5, 1, st))
            refused("groups of 4|channel/group", lib.quber_op_gn_apply(p, 8, 0, es, q, cs, 0, es, 1, 2, 2, c, 1, 2, ptr(stats), p, p, 8, 1e-5, 1, st))
            refused("groups of 4", lib.quber_op_maxpool_view(q, cs, 0, es, p, 8, 0, es, 1, 4, 4, c, 1, st))
            refused("groups of 4", lib.quber_op_maxpool_view(p, 8, 0, es, q, cs, 0, es, 1, 4, 4, c, 1, st))
            refused("groups of 4", lib.quber_op_bilinear_view(q, cs, es, p, 8, es, 1, 2, 2, c, 4, 4, st))
            refused("groups of 4", lib.quber_op_bilinear_view(p, 8, es, q, cs, es, 1, 2, 2, c, 4, 4, st))
            refused("groups of 4", lib.quber_op_avgpool(q, cs, es, p, 8, es, 1, 2, 2, c, st))
            refused("groups of 4", lib.quber_op_add_channels(q, cs, es, p, 8, es, p, 8, es, 1, 2, 2, c, st))
            refused("groups of 4", lib.quber_op_add_channels(p, 8, es, q, cs, es, p, 8, es, 1, 2, 2, c, st))
            refused("groups of 4", lib.quber_op_add_channels(p, 8, es, p, 8, es, q, cs, es, 1, 2, 2, c, st))
            refused("groups of 4", lib.quber_op_copy_channels(q, cs, es, p, 8, es, 1, 2, 2, c, st))
            refused("groups of 4", lib.quber_op_copy_channels(p, 8, es, q, cs, es, 1, 2, 2, c, st))
        refused("groups of 4", lib.quber_op_maxpool_view(p, 8, 6, es, p, 8, 0, es, 1, 4, 4, 8, 2, st))          # gs = 6
        refused("groups of 4", lib.quber_op_preprocess(p, p, p, p, 6, es, 1, 1, 2, 2, (C.c_float * 6)(), (C.c_float * 6)(*[1] * 6), 2, st))
        refused("groups of 4", lib.quber_op_preprocess(p, p, p, p2, 8, es, 1, 1, 2, 2, (C.c_float * 6)(), (C.c_float * 6)(*[1] * 6), 2, st))
    refused("capacity", lib.quber_op_preprocess(p, p, p, p, 8, 4, 2, 1, 2, 2, (C.c_float * 6)(), (C.c_float * 6)(*[1] * 6), 2, st))
    refused("channel/group", lib.quber_op_gn_stats(p, 48, 0, 4, 1, 2, 2, 48, 1, 32, ptr(stats), 1, st))          # 48 channels in 32 groups
    PA, IA = C.c_void_p * 6, C.c_int32 * 6
    ptrs, ones, zeros = PA(*[p.value] * 6), IA(*[1] * 6), IA(*[0] * 6)

    def pred(n=1, c=32, cs=32, es=4, feat=ptrs, cout=ones, q0=zeros, q_nch=4):
        return lib.quber_op_predictors(n, feat, ptrs, ptrs, PA(), cout, q0, zeros, c, cs, es, 1, 2, 2, p, q_nch, 8, st)

    refused("32 or 64 input channels and 1..5 heads", pred(n=6))
    refused("32 or 64 input channels and 1..5 heads", pred(n=0))
    refused("32 or 64 input channels and 1..5 heads", pred(c=48, cs=48))
    refused("outputs per head", pred(cout=IA(*[5] * 6)))
    refused("outputs per head", pred(cout=zeros))
    refused("outside q", pred(cout=IA(*[2] * 6), q0=IA(*[3] * 6)))
    refused("groups of 4", pred(cs=34))
    refused("groups of 4", pred(feat=PA(*[p2.value] * 6)))
    refused("groups of 4", pred(es=2, feat=PA(*[p2.value] * 6)))
    assert (get().view(np.uint32) == 0xA5A5A5A5).all()
