"""GPU: the tile-to-tile pipeline of the persistent LDS-DMA convolution kernels (csrc/conv_h8.hip: conv_h8 / h8n / h8p / h8w / h8s kernels;
csrc/conv_x8.hip) on launches whose blocks really WALK: every block computes three or four tiles, and from one tile of a run to the next the
channel tile (and so the scale / shift vectors the kernel fetched a tile ahead), the image or both change.  tests/tile_walks.py is the host model
of the walks; its facts are preconditions here, evaluated with the device's CU count (tests/test_tile_walks_model.py holds them at 256 blocks).

Through the C ABI only (quber_op_conv2d_f16; quber_op_conv2d in the bf16x3 mode), against a float64 CPU convolution of the same fp16 / fp32
operands (the oracle's arithmetic for one layer: oracle/network_torch.py runs the reference's F.conv2d) and against the 128-tile kernels the
LDS-DMA kernels replace (conv_igemm.hip: option key 31 = 0 / key 35 = 0).  Bars: those of tests/test_gpu_h8.py (fp16: 3e-3 of the output scale
- one fp16 rounding of an fp32 sum over K <= 4608) and tests/test_gpu_x8.py (bf16x3: 2e-6 of the output scale).

Operands: scale and shift carry a signature per channel tile - tile 0 scale +1 / shift 0, tile 1 scale -1.5 / shift +2, tile 2 scale +0.5 /
shift -2 (+-25 % and +-0.3 of per-channel noise) - so an output computed with the vectors of another channel tile, or with a mix of two, is
off by O(1): two orders above the fp16 bar.  The shift noise of a norm group's channels is 0.1 ... 0.3 with ONE sign, that of the group's mean
signature shift, so no group's mean is near zero (asserted: above 0.05; 0.13 and more in the table cases) and the RELATIVE bar of the
GroupNorm sums (2e-6, as tests/test_gpu_h8.py) governs: with 2.6e5 values and more per (image, group) it is 2.6e-2 and more, against
differences of 1e-8 relative measured (profiles/tile_walks.md).  The absolute term stays 1e-4: it does not grow with the images."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tile_walks as tw
from quber_amd import _lib
from test_gpu_h8 import pack

pytestmark = pytest.mark.gpu

SIGNATURE = ((1.0, 0.0), (-1.5, 2.0), (0.5, -2.0), (1.25, 1.0), (-0.75, 3.0))      # (scale, shift) of channel tile 0, 1, 2, ... (3, 4: the random walks)
_P = lambda t_: C.c_void_p(t_.data_ptr()) if t_ is not None else None


@functools.lru_cache(None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(None)
def _engine():
    """A context without a network: its stage profile records the stand-alone launches of this thread."""
    from quber_amd import engine
    return engine.Engine(engine.make_config(height=32, width=32, with_network=False), "cuda:0")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def operands(c, width, seed, fp16):
    """-> x [B][H][W][cin], w OIHW, scale, shift, residual (CPU; fp16: the tensors rounded to fp16).  width: channels per channel tile."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((c.B, c.H, c.W, c.cin), generator=g)
    w = torch.randn((c.cout, c.cin, c.k, c.k), generator=g) / (c.cin * c.k * c.k) ** 0.5
    scale = shift = None
    if c.affine:
        tile = torch.arange(c.cout) // width
        sig = torch.tensor(SIGNATURE)[tile]
        scale = sig[:, 0] * (1 + 0.25 * (2 * torch.rand(c.cout, generator=g) - 1))
        cpg = c.cout // c.groups if c.groups else 1
        # one noise sign per norm group: that of the group's mean signature shift (a group can straddle two channel tiles), so the noise moves
        # the group's mean away from zero; groups of mean 0 (channel tile 0) alternate
        gmean = sig[:, 1].reshape(-1, cpg).mean(1)
        sign = torch.where(gmean == 0, torch.where(torch.arange(c.cout // cpg) % 2 == 0, 1.0, -1.0), torch.sign(gmean)).repeat_interleave(cpg)
        shift = sig[:, 1] + sign * (0.1 + 0.2 * torch.rand(c.cout, generator=g))
    oh, ow = tw.out_size(c)
    res = torch.randn((c.B, oh, ow, c.cout), generator=g) if c.residual else None
    if fp16:
        x, w, res = x.half(), w.half(), res.half() if res is not None else None
    return x, w, scale, shift, res


def reference(c, x, w, scale, shift, res):
    """float64 on the CPU, from the operands as the kernel reads them."""
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, c.stride, c.pad, c.dil).permute(0, 2, 3, 1).contiguous()
    if c.affine:
        ref = ref * scale.double() + shift.double()
    if res is not None:
        ref = ref + res.double()
    return ref.clamp_min(0) if c.relu else ref


def launch_f16(lib, c, xd, wd, sd, hd, rd):
    oh, ow = tw.out_size(c)
    y = torch.full((c.B, oh, ow, c.cout), float("nan"), dtype=torch.float16, device="cuda")
    sums = torch.zeros((c.B, c.groups, 2), dtype=torch.float64, device="cuda") if c.groups else None
    _lib.check(lib.quber_op_conv2d_f16(_P(xd), c.B, c.H, c.W, c.cin, _P(wd), c.cout, c.k, c.stride, c.pad, c.dil, c.kmode, _P(sd), _P(hd), _P(rd),
                                       int(c.relu), _P(sums), c.groups, _P(y), _stream()))
    torch.cuda.synchronize()
    return y, sums


def launch_f32(lib, c, xd, wd, sd, hd, rd, scratch):
    oh, ow = tw.out_size(c)
    y = torch.full((c.B, oh, ow, c.cout), float("nan"), device="cuda")
    _lib.check(lib.quber_op_conv2d(_P(xd), c.B, c.H, c.W, c.cin, _P(wd), c.cout, c.k, c.stride, c.pad, c.dil, _P(sd), _P(hd), _P(rd), int(c.relu),
                                   _P(scratch), _P(y), _stream()))
    torch.cuda.synchronize()
    return y, None


def profiled(fn):
    """fn() inside a stage-profile window -> (its result, {stage: launches})."""
    e = _engine()
    e.profile_begin()
    try:
        out = fn()
    finally:
        stages = e.profile_end()
    return out, {k: v["launches"] for k, v in stages.items()}


def first_index(bad):
    """bad: a bool tensor [B][oh][ow][cout] with at least one True -> the (b, oy, ox, channel) of the first."""
    return tuple(int(v) for v in np.unravel_index(int(bad.reshape(-1).to(torch.uint8).argmax()), tuple(bad.shape)))


def max_abs_diff(a, b, chunks=16):
    """max |a - b| in float64 and its index, slice by slice (b: a device tensor or the float64 reference on the CPU - moved over a slice at a
    time, so that a launch's device footprint stays its operands and outputs)."""
    shape, a, b = tuple(a.shape), a.reshape(-1), b.reshape(-1)
    n = a.numel()
    step = -(-n // chunks)
    best, at = -1.0, 0
    for lo in range(0, n, step):
        d = (a[lo:lo + step].double() - b[lo:lo + step].cuda().double()).abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        i = int(d.argmax())
        if float(d[i]) > best:
            best, at = float(d[i]), lo + i
    return best, tuple(int(v) for v in np.unravel_index(at, shape))


def where(c, family, index):
    """The walk model's words on output element index = (b, oy, ox, channel)."""
    return tw.describe(c, index[:3], index[3], _cus(), family)


def check_walks(c, family):
    """The model's preconditions for this device; skips (other CU counts only) when the launch does not walk."""
    geo = tw.geometry(c, family)
    k = tw.classify(tw.walk(c, _cus(), family))
    ok = set(k["lengths"]) <= {3, 4}
    if geo["ntiles"] > 1:
        ok = ok and k["pairs"]["channel_tile"] >= 300 and k["triples"]["channel_tile"] >= 200
    else:
        ok = ok and k["pairs"]["image"] >= 32
    if not ok and _cus() != 256:
        pytest.skip(f"case {c.id} does not walk on {_cus()} CUs: {k}")
    assert ok, (c.id, family, k)
    return geo, k


def stored_sums(y, groups):
    """float64 sums and sums of squares of the stored outputs per (image, norm group), an image at a time -> [B][groups][2]."""
    out = []
    for yb in y:
        yd = yb.double().reshape(-1, groups, yb.shape[-1] // groups)
        out.append(torch.stack([yd.sum((0, 2)), (yd * yd).sum((0, 2))], -1))
    return torch.stack(out)


def check_case(c, family, fp16, keys, stage, seed=None, what=""):
    """One launch geometry on one kernel, the six assertions of the table cases: (1) finite and float64-close, (2) three launches bit-equal, (3) the
    replaced kernel inside the same bar and the two within it of each other, (4) the norm sums, (5) the routing, (6) a walk-model message on failure.
    keys: {option key: value} of the kernel meant; the replaced kernel is the same launch with key 31 (fp16) / 35 (bf16x3) = 0."""
    lib = _lib.load()
    geo = tw.geometry(c, family)
    lengths = sorted({len(r) for r in tw.walk(c, _cus(), family)})
    x, w, scale, shift, res = operands(c, geo["width"], 4321 + c.cin + c.cout + c.k if seed is None else seed, fp16)
    ref = reference(c, x, w, scale, shift, res)
    dev = lambda t_: t_.cuda() if t_ is not None else None
    if fp16:
        args = (dev(x), dev(pack(w, c.kmode)), dev(scale), dev(shift), dev(res))
        go, off_key, rel = (lambda: launch_f16(lib, c, *args)), 31, 3e-3
    else:
        args = (dev(x), dev(w), dev(scale), dev(shift), dev(res), torch.empty(c.cout * c.cin * c.k * c.k, device="cuda"))
        go, off_key, rel = (lambda: launch_f32(lib, c, *args)), 35, 2e-6
    del x, w, res
    defaults = {12: 0, 31: 1, 35: 1, 38: 1}
    differ = None
    try:
        for key, v in keys.items():
            lib.quber_set_tuning(key, v)
        (y, sums), stages = profiled(go)
        for _ in range(2):
            other = go()[0]
            if differ is None and not torch.equal(y, other):
                differ = first_index(y != other)
        del other
        lib.quber_set_tuning(off_key, 0)
        (y0, sums0), stages0 = profiled(go)
    finally:
        for key in set(keys) | {off_key}:
            lib.quber_set_tuning(key, defaults[key])
    tol = rel * max(1.0, float(ref.abs().max()))
    (e, at), (e0, _), (ab, at_ab) = max_abs_diff(y, ref), max_abs_diff(y0, ref), max_abs_diff(y, y0)
    gn = ""
    if c.groups:
        exp = stored_sums(y, c.groups)
        mean = float(exp[..., 0].abs().min()) / (y[0].numel() // c.groups)
        gn = f"sums: abs {float((sums - exp).abs().max()):.3e} rel {float(((sums - exp).abs() / exp.abs()).max()):.3e} least |mean| {mean:.3f} "
    print(f"tile walk {c.id} [{family}] {what}tiles {geo['tiles']} runs {lengths}: err {e:.3e} replaced {e0:.3e} between {ab:.3e} bar {tol:.3e} "
          f"repeats {'differ' if differ else 'equal'} {gn}stages {stages} / {stages0}")
    # 5. the kernel meant really ran: one launch under its stage and none of the 128-tile kernel; none of its own with the key off
    # (a stage an earlier window recorded stays listed, with 0 launches)
    assert stages.get(stage) == 1 and not stages.get("conv_gemm"), (c.id, what, stages)
    assert not any(n for s, n in stages0.items() if s.endswith(("_h8", "_x8"))), (c.id, what, stages0)
    # 1. finite, float64-close (6: the message names the tile, its block and the run's neighbours)
    finite = torch.isfinite(y)
    assert bool(finite.all()), what + "not finite: " + where(c, family, first_index(~finite))
    assert e < tol, what + f"{e:.3e} >= {tol:.3e}: " + where(c, family, at)
    # 2. no data-dependent control in the pipeline: any run-to-run difference is a race between a DMA and a read
    assert differ is None, what + "launches differ: " + where(c, family, differ or at)
    # 3. the kernel it replaces: the same bar, and the two within it of each other
    assert e0 < tol, (c.id, what, e0, tol)
    assert ab < tol, what + f"{ab:.3e} >= {tol:.3e} between the kernels: " + where(c, family, at_ab)
    # 4. the GroupNorm sums of the STORED outputs
    if c.groups:
        assert mean > 0.05, (c.id, what, mean)                   # (the operands' doing: the relative bar governs)
        bad = ~torch.isclose(sums, exp, rtol=2e-6, atol=1e-4)
        assert not bool(bad.any()), (c.id, what, gn, bad.nonzero()[:8].tolist())
        assert torch.allclose(sums0, stored_sums(y0, c.groups), rtol=1e-11, atol=1e-9), (c.id, what)


@pytest.mark.parametrize("cid", [c.id for c in tw.TABLE if c.family != "x8"])
def test_fp16_kernels_on_runs_of_three_and_four_tiles(cid):
    c = tw.BY_ID[cid]
    check_walks(c, tw.launched_family(c))
    check_case(c, tw.launched_family(c), True, {}, "conv_gemm_h8")


@pytest.mark.parametrize("cid", ["A", "B"])
def test_wide_3x3_layers_walk_the_gather_kernel_with_key_38_at_2(cid):
    """The same layers on conv_h8_kernel's 256-row tiles (case A runs there at any key 38: conv_h8w_kernel takes no launch of one channel block)."""
    c = tw.BY_ID[cid]
    assert tw.launched_family(c, key38=2) == "h8"
    check_walks(c, "h8")
    check_case(c, "h8", True, {38: 2}, "conv_gemm_h8")


@pytest.mark.parametrize("cid", ["H", "I"])
def test_bf16x3_kernel_on_runs_of_three_and_four_tiles(cid):
    c = tw.BY_ID[cid]
    check_walks(c, "x8")
    check_case(c, "x8", False, {12: 3}, "conv_gemm_x8")          # key 35 at its default: both launches pass its gates (9 K-slices, 3 rounds of tiles)


@pytest.mark.parametrize("it", range(12))
def test_random_walks_are_deterministic_and_match(it):
    """Randomised launches as test_gpu_h8.py's fuzz draws them (ragged pixel and channel tiles, dilation, stride, every epilogue variant; odd
    launches with key 38 = 2), but every one of 3 - 5 tiles per block and 1, 2, 3 or 5 channel tiles: float64, three launches, the 128-tile kernel."""
    c, key38 = tw.random_walks(_cus())[it]
    geo = tw.geometry(c)
    runs = tw.walk(c, _cus())
    assert 3 * _cus() + 1 <= geo["tiles"] <= 5 * _cus() and {len(r) for r in runs} <= {3, 4, 5}, (c, geo)
    check_case(c, c.family, True, {38: key38}, "conv_gemm_h8", seed=7000 + it, what=f"k{c.k} {c.cin}>{c.cout} B{c.B} {c.H}x{c.W} d{c.dil} s{c.stride} key 38 = {key38}: ")
