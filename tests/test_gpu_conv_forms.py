"""GPU: the convolution kernels on their own in the forms the plan launches them (csrc/plan.hip emit_conv) - several launch groups, channel-slice
views with group strides, GroupNorm sums gathered by the convolution, the norm in front of a Winograd layer applied on load - through the view
forms of the stand-alone ops (quber_op_conv2d_view, quber_op_conv3x3_winograd_view, quber_op_conv1x1_dual_view), exact fp32 and bf16x3.

The rows are tests/conv_forms.py; each test first asserts, from the launchers' own report (quber_debug_*_route), that its row takes the route it names.

Every destination is a sentinel-filled slab of one frame more than the batch, every source slab holds 1e3 +- 50 outside its view, the sums sit between
guards; every row asserts that no byte outside the destination view changed.

Bounds (the project's own, nothing tuned here):
  output   against the float64 convolution (torch.nn.functional.conv2d on the CPU, per group, + affine, residual, ReLU) of the same fp32 data, as
           max |error| / max(1, max |reference|): < 2e-6 (test_conv_igemm_vs_torch; bf16x3: test_conv_igemm_bf16x3_meets_the_fp32_bar; the dual GEMM:
           test_conv1x1_dual_vs_torch), Winograd {2: 1e-5, 4: 2e-5, 6: 1e-4} (test_conv3x3_winograd_vs_float64).  The full tensor.
  bits     a grouped / sliced launch equals G launches of the dense op on the same data bit for bit where the K order of an element cannot depend on
           G: forced tile shape and K partitions without the persistent kernel, and both Winograd forms.  Persistent launches (and conv_x8, whose
           tile walk is persistent too) share remainder tiles by the tile count of the whole launch: only the float64 bar applies there.
  sums     against the float64 sums and sums of squares of the STORED output, per (launch group, image, norm group): 2 n 2^-53 sum |terms|,
           n = OH OW channels per group (the bound of test_groupnorm: every term is formed in double from a float).  Once into a cleared buffer,
           once more into a buffer pre-loaded with known values: the launch accumulates (bound + 2 n 2^-53 |pre-load| for the extra additions)
           and every other slot keeps its value.
  norm     normalise-on-load equals quber_op_gn_apply into a temporary followed by the same launch without the norm, bit for bit: both evaluate
           fmaxf(fmaf(x, rstd gamma, beta - mean rstd gamma), lo) from the same sums (elementwise.hip gn_apply_kernel, winograd.hip wino_input_kernel,
           wino_fused.hip wino_norm_coef_kernel); a padding tap contributes 0, not norm(0)."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import conv_forms as cf
from quber_amd import _lib
from test_gpu_glue import F64, Slab, assert_bits, guarded, ptr, stream

pytestmark = pytest.mark.gpu

NULL = C.c_void_p(0)
WINO_TOL = {2: 1e-5, 4: 2e-5, 6: 1e-4}


def P(t):
    return ptr(t) if t is not None else NULL


def dev(t):
    return t.contiguous().cuda()


def gen(c):
    return torch.Generator().manual_seed(zlib.crc32(c.id.encode()))


def nhwc(t):
    """[G][B][C][H][W] -> numpy [G][B][H][W][C]"""
    return t.permute(0, 1, 3, 4, 2).contiguous().numpy()


def sums_buffer(values):
    """device f64 buffer holding `values` between two sentinel guards: (tensor, pointer to the payload, checker returning the payload)"""
    t, off, payload = guarded(values.size, F64)
    t[off:off + values.size * 8] = torch.from_numpy(np.ascontiguousarray(values, F64).reshape(-1).view(np.uint8)).cuda()
    return t, ptr(t, off), payload


def check_output(name, got, ref, bar):
    """got, ref [G][B][H][W][C]; the existing tests' measure: max |error| / max(1, max |reference|)"""
    err = float(np.abs(got.astype(F64) - ref).max()) / max(1.0, float(np.abs(ref).max()))
    print(f"{name}: output {err:.3e} = {err / bar:.3f} of the bar {bar:g}")
    assert np.isfinite(got).all() and err < bar, (name, err, bar)


def stored_sums(got, groups):
    """float64 sums, sums of squares and sums of |terms| of the stored output [G][B][H][W][C] per (g, b, norm group)"""
    G_, B, H, W, C_ = got.shape
    v = got.astype(F64).reshape(G_, B, H * W, groups, C_ // groups)
    s, q = v.sum((2, 4)), (v * v).sum((2, 4))
    return np.stack([s, q], -1), np.stack([np.abs(v).sum((2, 4)), q], -1), H * W * (C_ // groups)


def check_sums(name, launch, ys, B, groups, G_):
    """launch(sums pointer) runs the row; returns the stored output of the first launch"""
    n_slots = G_ * B * groups * 2
    t0, p0, read0 = sums_buffer(np.zeros(n_slots))
    launch(p0)
    got = ys.fetch(B)
    want, mag, n = stored_sums(got, groups)
    bound = 2.0 * n * 2.0 ** -53 * mag
    s0 = read0().reshape(want.shape)
    r0 = float((np.abs(s0 - want) / np.maximum(bound, 1e-300)).max())
    pre = (np.arange(n_slots, dtype=F64) * 0.37 - 11.0).reshape(want.shape) * 1e3
    t1, p1, read1 = sums_buffer(pre)
    launch(p1)
    again = ys.fetch(B)
    s1 = read1().reshape(want.shape)
    bound1 = bound + 2.0 * n * 2.0 ** -53 * np.abs(pre)
    r1 = float((np.abs(s1 - (pre + want)) / bound1).max())
    print(f"{name}: sums {r0:.3f} of the bound into a cleared buffer, {r1:.3f} into a pre-loaded one (n = {n})")
    bad = np.argwhere(np.abs(s0 - want) > bound)
    assert bad.size == 0, (name, "sums", bad[0], s0[tuple(bad[0])], want[tuple(bad[0])])
    bad = np.argwhere(np.abs(s1 - (pre + want)) > bound1)
    assert bad.size == 0, (name, "accumulated sums", bad[0], s1[tuple(bad[0])], (pre + want)[tuple(bad[0])])
    assert_bits(again, got, name + ": second launch")
    return got


# ------------------------------------------------------------------------------------------------------------------------------------
# implicit GEMM: one tile per block, split-K, persistent, conv_x8

def conv_reference(c):
    g = gen(c)
    x = torch.randn(c.G, c.B, c.cin, c.H, c.W, generator=g)
    w = torch.randn(c.G, c.cout, c.cin, c.k, c.k, generator=g) / np.sqrt(c.cin * c.k * c.k)
    sc = torch.rand(c.G, c.cout, generator=g) + 0.5 if c.affine else None
    sh = torch.randn(c.G, c.cout, generator=g) if c.affine else None
    oh, ow = cf.out_hw(c)
    res = torch.randn(c.G, c.B, c.cout, oh, ow, generator=g) if c.res else None
    ref = torch.stack([torch.nn.functional.conv2d(x[i].double(), w[i].double(), None, c.stride, c.pad, c.dil) for i in range(c.G)])
    if c.affine:
        ref = ref * sc.double().view(c.G, 1, -1, 1, 1) + sh.double().view(c.G, 1, -1, 1, 1)
    if c.res:
        ref = ref + res.double()
    if c.relu:
        ref = ref.relu()
    return x, w, sc, sh, res, nhwc(ref)


@pytest.mark.parametrize("c", cf.CONV_CASES, ids=[c.id for c in cf.CONV_CASES])
def test_conv_view_forms(c):
    lib = _lib.load()
    r = cf.conv_route(lib, c, device=True)
    assert (r.kernel, r.sums, r.BM, r.BN, r.S, r.tail) == (c.kernel, c.sums, c.BM, c.BN, c.S, c.tail), r
    x, w, sc, sh, res, ref = conv_reference(c)
    oh, ow = cf.out_hw(c)
    Bcap = c.B + cf.BCAP_EXTRA
    rng = np.random.default_rng(1)
    xs = Slab(4, c.G, Bcap, c.H, c.W, c.cin + c.in_pad, 0, c.cin, rng).put(nhwc(x))
    rs = Slab(4, c.G, Bcap, oh, ow, c.cout + 4, 4, c.cout, rng).put(nhwc(res)) if c.res else None
    ys = Slab(4, c.G, Bcap, oh, ow, c.cout + c.out_pad, c.c0, c.cout).up()
    assert (xs.cs, xs.gs, ys.cs, ys.gs) == cf.conv_strides(c, Bcap)
    wd, scd, shd = dev(w), dev(sc) if c.affine else None, dev(sh) if c.affine else None
    kpad = (c.k * c.k * c.cin + 31) // 32 * 32
    packed = torch.empty(c.G * c.cout * kpad, device="cuda")

    def launch(sums):
        _lib.check(lib.quber_op_conv2d_view(xs.p, xs.cs, xs.gs, P(wd), P(scd), P(shd), rs.p if rs else NULL, rs.cs if rs else 0, rs.gs if rs else 0, ys.p,
                                            ys.cs, ys.gs, c.G, c.B, c.H, c.W, c.cin, c.cout, c.k, c.stride, c.pad, c.dil, int(c.relu), sums, c.groups,
                                            P(packed), stream()))
    rd = cf.conv_route(lib, c._replace(G=1, in_pad=0, out_pad=0, c0=0, groups=0), device=True)        # the dense op's route, one group at a time
    with cf.keys_set(lib, c.keys, True):
        if c.out_pad % 4:
            # Scalar stores (a pixel stride off the 16-byte grid): the sums go to the separate pass, and that pass takes aligned groups of four
            # channels only - the launcher's own refusal, after a convolution that is right and stays inside its view.  (The plan never builds
            # such a view: every slab it allocates has a multiple of 4 channels.)
            t0, p0, read0 = sums_buffer(np.zeros(c.G * c.B * c.groups * 2))
            with pytest.raises(_lib.QuberError, match="aligned groups of 4"):
                launch(p0)
            check_output(c.id, ys.fetch(c.B), ref, 2e-6)
            assert not read0().any()
            return
        got = check_sums(c.id, launch, ys, c.B, c.groups, c.G)
        check_output(c.id, got, ref, 2e-6)
        if c.kernel in ("tile", "splitk"):
            # the dense op, one group at a time: the same tile shape and K partitions (asserted), so the same K order per element
            assert (rd.kernel, rd.BM, rd.BN, rd.S, rd.tail) == (r.kernel, r.BM, r.BN, r.S, r.tail), rd
            for g in range(c.G):
                xd, yd = dev(torch.from_numpy(nhwc(x)[g])), torch.empty(c.B, oh, ow, c.cout, device="cuda")
                resd = dev(torch.from_numpy(nhwc(res)[g])) if c.res else None
                wg, scg, shg = dev(w[g]), dev(sc[g]) if c.affine else None, dev(sh[g]) if c.affine else None
                _lib.check(lib.quber_op_conv2d(P(xd), c.B, c.H, c.W, c.cin, P(wg), c.cout, c.k, c.stride, c.pad, c.dil, P(scg), P(shg), P(resd), int(c.relu),
                                               P(packed), P(yd), stream()))
                torch.cuda.synchronize()
                assert_bits(got[g], yd.cpu().numpy(), f"{c.id}: group {g} against the dense op")


# ------------------------------------------------------------------------------------------------------------------------------------
# Winograd: the three-kernel pipeline and the single kernel

def wino_reference(c):
    g = gen(c)
    Gx = 1 if c.shared else c.G
    x = torch.randn(Gx, c.B, c.cin, c.H, c.W, generator=g)
    if c.norm:
        x = 1.0 + 3.0 * x
    w = torch.randn(c.G, c.cout, c.cin, 3, 3, generator=g) / np.sqrt(c.cin * 9)
    sc = torch.rand(c.G, c.cout, generator=g) + 0.5 if c.affine else None
    sh = torch.randn(c.G, c.cout, generator=g) if c.affine else None
    gamma = torch.rand(c.G, c.cin, generator=g) + 0.5 if c.norm else None
    beta = torch.randn(c.G, c.cin, generator=g) if c.norm else None
    refs = []
    for i in range(c.G):
        xi = x[0 if c.shared else i].double()
        if c.norm:
            v = xi.reshape(c.B, c.norm_groups, -1)
            mean, var = v.mean(2, keepdim=True), v.var(2, unbiased=False, keepdim=True)
            xi = ((v - mean) / torch.sqrt(var + 1e-5)).reshape(xi.shape) * gamma[i].double().view(1, -1, 1, 1) + beta[i].double().view(1, -1, 1, 1)
            if c.norm_relu:
                xi = xi.relu()
        refs.append(torch.nn.functional.conv2d(xi, w[i].double(), None, 1, c.dil, c.dil))
    ref = torch.stack(refs)
    if c.affine:
        ref = ref * sc.double().view(c.G, 1, -1, 1, 1) + sh.double().view(c.G, 1, -1, 1, 1)
    if c.relu:
        ref = ref.relu()
    return x, w, sc, sh, gamma, beta, nhwc(ref)


@pytest.mark.parametrize("c", cf.ALL_WINO, ids=[c.id for c in cf.ALL_WINO])
def test_winograd_view_forms(c):
    lib = _lib.load()
    r = cf.wino_route(lib, c, device=True)
    assert (r.kernel, r.sums, r.BM, r.S) == (c.kernel, c.sums, c.per_block, c.passes), r
    x, w, sc, sh, gamma, beta, ref = wino_reference(c)
    Bcap, Gx = c.B + cf.BCAP_EXTRA, 1 if c.shared else c.G
    rng = np.random.default_rng(2)
    Pn = (c.m + 2) ** 2
    wd, scd, shd = dev(w), dev(sc) if c.affine else None, dev(sh) if c.affine else None
    u = torch.empty(c.G * Pn * c.cout * c.cin, device="cuda")
    ws = torch.empty(cf.wino_ws_floats(c), device="cuda")
    gd, bd = (dev(gamma), dev(beta)) if c.norm else (None, None)

    def slabs():
        xs = Slab(4, Gx, Bcap, c.H, c.W, c.cin + c.in_pad, 0, c.cin, rng).put(nhwc(x))
        ys = xs if c.in_place else Slab(4, c.G, Bcap, c.H, c.W, c.cout + c.out_pad, c.c0, c.cout).up()
        return xs, ys
    xs, ys = slabs()
    x_gs = 0 if c.shared else xs.gs
    assert (xs.cs, x_gs, ys.cs, ys.gs) == cf.wino_strides(c, Bcap)
    stats = None
    if c.norm:      # the sums of the input, once, by the stats pass: one copy per launch group (a shared input: G identical ones)
        stats = torch.zeros(c.G * c.B * c.norm_groups * 2, dtype=torch.float64, device="cuda")
        _lib.check(lib.quber_op_gn_stats(xs.p, xs.cs, x_gs, 4, c.B, c.H, c.W, c.cin, c.G, c.norm_groups, P(stats), 1, stream()))

    def run(src, src_gs, dst, sums, with_norm):
        _lib.check(lib.quber_op_conv3x3_winograd_view(src.p, src.cs, src_gs, P(wd), P(scd), P(shd), dst.p, dst.cs, dst.gs, c.G, c.B, c.H, c.W, c.cin, c.cout,
                                                      c.dil, c.m, int(c.relu), sums, c.groups, P(stats) if with_norm else NULL, P(gd) if with_norm else NULL,
                                                      P(bd) if with_norm else NULL, c.cin, c.norm_groups, c.norm_relu, 1e-5, P(u), P(ws), ws.numel(), stream()))
    with cf.keys_set(lib, c.keys, True):
        if c.in_place:
            # the input is consumed: one launch into a cleared buffer (accumulation is covered by the other rows)
            t0, p0, read0 = sums_buffer(np.zeros(c.G * c.B * c.groups * 2))
            run(xs, x_gs, ys, p0, True)
            got = ys.fetch(c.B)
            want, mag, n = stored_sums(got, c.groups)
            ratio = float((np.abs(read0().reshape(want.shape) - want) / (2.0 * n * 2.0 ** -53 * mag)).max())
            print(f"{c.id}: sums {ratio:.3f} of the bound (in place)")
            assert ratio <= 1.0
        else:
            got = check_sums(c.id, lambda sums: run(xs, x_gs, ys, sums, c.norm), ys, c.B, c.groups, c.G)
        check_output(c.id, got, ref, WINO_TOL[c.m])
        if c.norm:
            # the norm as the pass it was, into a temporary, then the same launch without it
            ts = Slab(4, c.G, Bcap, c.H, c.W, c.cin, 0, c.cin).up()
            xs2, _ = slabs() if c.in_place else (xs, None)
            _lib.check(lib.quber_op_gn_apply(xs2.p, xs2.cs, x_gs, 4, ts.p, ts.cs, ts.gs, 4, c.B, c.H, c.W, c.cin, c.G, c.norm_groups, P(stats), P(gd), P(bd),
                                             c.cin, 1e-5, c.norm_relu, stream()))
            ts.fetch(c.B)
            y2 = Slab(4, c.G, Bcap, c.H, c.W, c.cout + c.out_pad, c.c0, c.cout).up()
            run(ts, ts.gs, y2, NULL, False)
            assert_bits(got, y2.fetch(c.B), f"{c.id}: normalise-on-load against the norm pass + the same launch")
        else:
            # the dense op, one group at a time
            for g in range(c.G):
                xd, yd = dev(torch.from_numpy(nhwc(x)[0 if c.shared else g])), torch.empty(c.B, c.H, c.W, c.cout, device="cuda")
                wg, scg, shg = dev(w[g]), dev(sc[g]) if c.affine else None, dev(sh[g]) if c.affine else None
                _lib.check(lib.quber_op_conv3x3_winograd(P(xd), c.B, c.H, c.W, c.cin, P(wg), c.cout, c.dil, c.m, P(scg), P(shg), int(c.relu), P(u), P(ws),
                                                         ws.numel(), P(yd), stream()))
                torch.cuda.synchronize()
                assert_bits(got[g], yd.cpu().numpy(), f"{c.id}: group {g} against the dense op")


# ------------------------------------------------------------------------------------------------------------------------------------
# the dual 1x1 GEMM of the projection blocks

@pytest.mark.parametrize("c", cf.DUAL_CASES, ids=[c.id for c in cf.DUAL_CASES])
def test_dual_view_forms(c):
    """Two groups at once against float64.  No comparison in bits with two dense launches: the dual GEMM is always a persistent launch (or conv_x8's
    persistent tile walk), whose remainder shares depend on the tile count of the whole launch."""
    lib = _lib.load()
    r = cf.dual_route(lib, c, device=True)
    assert (r.kernel, r.BM) == (c.kernel, c.BM), r
    g = gen(c)
    h2, w2 = (c.oh - 1) * c.stride + 1, (c.ow - 1) * c.stride + 1
    y = torch.randn(c.G, c.B, c.oh, c.ow, c.mid, generator=g)
    x = torch.randn(c.G, c.B, h2, w2, c.cin, generator=g)
    w = torch.randn(c.G, c.cout, c.mid + c.cin, generator=g) / np.sqrt(c.mid + c.cin)
    sh = torch.randn(c.G, c.cout, generator=g)
    ref = (torch.einsum("gbhwc,goc->gbhwo", y.double(), w[:, :, :c.mid].double()) +
           torch.einsum("gbhwc,goc->gbhwo", x[:, :, ::c.stride, ::c.stride].double(), w[:, :, c.mid:].double()) + sh.double().view(c.G, 1, 1, 1, -1))
    if c.relu:
        ref = ref.relu()
    Bcap = c.B + cf.BCAP_EXTRA
    rng = np.random.default_rng(3)
    ysl = Slab(4, c.G, Bcap, c.oh, c.ow, c.mid, 0, c.mid, rng).put(y.numpy())
    xsl = Slab(4, c.G, Bcap, h2, w2, c.cin, 0, c.cin, rng).put(x.numpy())
    out = Slab(4, c.G, Bcap, c.oh, c.ow, c.cout, 0, c.cout).up()
    wd, shd, ones = dev(w), dev(sh), torch.ones(c.G * c.cout, device="cuda")
    with cf.keys_set(lib, c.keys, True):
        _lib.check(lib.quber_op_conv1x1_dual_view(ysl.p, ysl.gs, xsl.p, xsl.gs, P(wd), c.cout * (c.mid + c.cin), P(shd), P(ones), c.cout, out.p, out.gs, c.G,
                                                  c.B, c.oh, c.ow, c.mid, h2, w2, c.cin, c.stride, c.cout, int(c.relu), stream()))
        check_output(c.id, out.fetch(c.B), ref.numpy(), 2e-6)
